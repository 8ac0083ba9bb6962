"""Records (or, with --check, replays) tests/golden/api_calls.json: what every pricing entry point of the C ABI returns and refuses.

Two kinds of case, each on a fresh handle, 3 instances and N = 4 on the strikes 90 / 100 / 110:

  results   a call through the public Python API, twice: the SHA-256 of every returned array's bytes, the full
            describe_last_sweep text and the deltas of graph_captures / graph_replays over the two calls.  "small" cases run
            50x25 (the whole loop in one small-grid launch), "stream" cases 100x30 with small_grid = 0 (the streaming time loop);
            `expect` is the piece of the description that shows it.
  refusals  one call through solver._lib (NULL pointers and broken structs included): (status, exact hadi_last_error text).  Every
            host-side refusal ahead of the sweep, the three statuses behind it, and the cases with two violations at once, whose
            winner is the order of the checks.

    python tools/record_api_calls.py [--lib other/libhadi.so] [--out file.json]   # record (the committed fixture: from the parent build)
    python tools/record_api_calls.py --check [--lib ...]                           # replay the committed fixture and compare

Recording twice and comparing (--against first.json) shows whether every hash is a property of the build.
tests/test_gpu_api_calls.py runs run_case() and compare() below, so the test and --check are one implementation.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "api_calls.json")

S_0, V_0, T, R_D, THETA, EPS = 100.0, 0.04, 1.0, 0.025, 0.8, 1e-6
RHO, SIGMA, KAPPA, ETA = -0.9, 0.3, 1.5, 0.04
STRIKES = [90.0, 100.0, 110.0]
N_STEPS = 4
# Dates that are paid on the 4 steps of 0.25: hadi_dividend_steps pays date t at the start of step n where n dt <= t < (n + 1) dt,
# and moves on to the next date once n dt has passed the current one -- 0.3 is paid at step 1, 0.8 at step 3 (under delta_t_i =
# 0.2 at steps 1 and 4, under 0.3 at step 1 alone: a table row per instance).  holds() requires every dividend case to differ from
# the same call without dividends.
DIVS = ([0.3, 0.8], [0.5, 0.3], [0.02, 0.02])
NO_DIVIDENDS = {"DIV": "EU", "AM_DIV": "AM"}
GRIDS = {"small": (50, 25, {}), "stream": (100, 30, {"small_grid": 0})}
EXPECT = {"small": "whole time loop in one launch", "stream": "row pass"}
SNAP = [2, 4]
SPOTS = {1: [80.0, 100.0, 123.4], 3: [[80.0, 100.0, 123.4], [70.5, 95.0, 130.0], [88.0, 110.0, 140.25]]}
SCALES = {1: [1.0, 0.5, 2.0], 3: [[1.0, 0.5, 2.0], [1.5, 1.0, 0.25], [0.75, 1.25, 1.0]]}
SCHED = {1: [2, 4], 3: [[1, 3], [2], [1, 2, 4]]}
BARRIER = dict(lower=60.0, upper=[150.0, 160.0, 170.0], rebate=1.0)
VARIANTS = {"EU": 0, "AM": 1, "DIV": 2, "AM_DIV": 3}
SUFFIX = {"EU": "", "AM": "_american", "DIV": "_dividends", "AM_DIV": "_american_dividends"}
# what a result case may leave out
DEFAULTS = {"kind": "result", "grid": "small", "mem": "host", "variant": "EU", "rows": 1, "dv": None, "v0i": 0, "dti": 0, "put": 0,
            "lad": 0, "r_f": 0.01}


def _result_cases():
    out = []

    def add(name, call, **kw):
        out.append(dict(name=name, call=call, **kw))

    add("do_small", "do")
    add("do_stream_device", "do", grid="stream", mem="device")
    add("do_am_small", "do", variant="AM")
    add("do_div_stream", "do", variant="DIV", grid="stream")
    add("do_am_div_small_device", "do", variant="AM_DIV", mem="device")
    add("do_div_stream_dti", "do", variant="DIV", grid="stream", dti=1)  # (delta_t_i: the dividend table has a row per instance)
    add("do_div_small_dti", "do", variant="DIV", dti=1)
    add("do_put_small", "do", put=1)
    add("pds_small", "pds")
    add("pds_stream_device", "pds", grid="stream", mem="device")
    for fam in ("bp", "jac"):
        add(fam + "_small_dv0", fam, dv=0)
        add(fam + "_stream_dv1_v0i", fam, grid="stream", dv=1, v0i=1)
        add(fam + "_am_stream_dv0", fam, variant="AM", grid="stream", dv=0)
        add(fam + "_div_small_dv1", fam, variant="DIV", dv=1)
        add(fam + "_am_div_stream_device", fam, variant="AM_DIV", grid="stream", mem="device", dv=1)
        add(fam + "_put_small_dv1", fam, put=1, dv=1)
    add("greeks_small", "greeks")
    add("greeks_ladder_stream", "greeks", grid="stream", lad=1)
    add("greeks_am_ladder_small_device", "greeks", variant="AM", lad=1, mem="device")
    add("ladder_small", "ladder", r_f=0.0)
    add("ladder_stream_dti", "ladder", grid="stream", dti=1, r_f=0.0)
    add("bp_ladder_stream_dv1_v0i", "bp_ladder", grid="stream", dv=1, v0i=1, r_f=0.0)
    add("bp_ladder_small_dv0_device", "bp_ladder", dv=0, mem="device", r_f=0.0)
    add("jac_ladder_small_dv1", "jac_ladder", dv=1, r_f=0.0)
    add("jac_ladder_stream_dv0", "jac_ladder", grid="stream", dv=0, r_f=0.0)
    add("sample_small_shared", "sample", r_f=0.0)
    add("sample_stream_rows_device", "sample", grid="stream", rows=3, mem="device", r_f=0.0)
    add("bp_samples_stream_shared_dv0", "bp_samples", grid="stream", dv=0, r_f=0.0)
    add("bp_samples_small_rows_dv1_v0i", "bp_samples", rows=3, dv=1, v0i=1, r_f=0.0)
    add("jac_samples_small_shared_dv1", "jac_samples", dv=1, r_f=0.0)
    add("jac_samples_stream_rows_dv0", "jac_samples", grid="stream", rows=3, dv=0, r_f=0.0)
    add("berm_small_shared", "berm")
    add("berm_stream_rows_device", "berm", grid="stream", rows=3, mem="device")
    add("berm_div_stream_shared", "berm", variant="DIV", grid="stream")
    add("bp_berm_stream_rows_dv1", "bp_berm", grid="stream", rows=3, dv=1)
    add("bp_berm_small_shared_dv0", "bp_berm", dv=0)
    add("jac_berm_small_rows_dv1", "jac_berm", rows=3, dv=1)
    add("jac_berm_stream_shared_dv0", "jac_berm", grid="stream", dv=0)
    add("barrier_small_shared", "barrier")
    add("barrier_stream_rows_device", "barrier", grid="stream", rows=3, mem="device")
    add("bp_barrier_stream_shared_dv1_v0i", "bp_barrier", grid="stream", dv=1, v0i=1)
    add("bp_barrier_small_rows_dv0", "bp_barrier", rows=3, dv=0)
    add("jac_barrier_small_shared_dv0", "jac_barrier", dv=0)
    add("jac_barrier_stream_rows_dv1", "jac_barrier", grid="stream", rows=3, dv=1)
    add("dbg_row_small", "dbg_row", expect="row pass")
    add("dbg_row_am_stream", "dbg_row", variant="AM", grid="stream")
    add("dbg_col_small", "dbg_col", expect="row pass")
    return out


# ---- refusals: the raw argument list of every entry point, by name -----------------------------------------------------------------
_PRICE, _JAC = ["S_0", "V_0", "out"], ["S_0", "V_0", "eps", "J", "base"]
SIG = {
    "hadi_DO_timestepping": [], "hadi_parallel_DO_solve": _PRICE, "hadi_compute_greeks": ["S_0", "V_0", "greeks", "lad"],
    "hadi_maturity_ladder": ["S_0", "V_0", "n_snap", "snap", "out"], "hadi_compute_base_prices_ladder": ["S_0", "V_0", "n_snap", "snap", "out"],
    "hadi_compute_jacobian_ladder": ["S_0", "V_0", "eps", "n_snap", "snap", "J", "base"],
    "hadi_sample_ladder": ["V_0", "samples", "n_snap", "snap", "out"], "hadi_compute_base_prices_samples": ["V_0", "samples", "n_snap", "snap", "out"],
    "hadi_compute_jacobian_samples": ["V_0", "eps", "samples", "n_snap", "snap", "J", "base"],
    "hadi_bermudan_timestepping": ["n_ex", "ex", "ex_rows"], "hadi_compute_base_prices_bermudan": ["S_0", "V_0", "n_ex", "ex", "ex_rows", "out"],
    "hadi_compute_jacobian_bermudan": ["S_0", "V_0", "eps", "n_ex", "ex", "ex_rows", "J", "base"],
    "hadi_barrier_timestepping": ["barrier"], "hadi_compute_base_prices_barrier": ["S_0", "V_0", "barrier", "out"],
    "hadi_compute_jacobian_barrier": ["S_0", "V_0", "eps", "barrier", "J", "base"],
    "hadi_debug_row_pass": ["step", "out"], "hadi_debug_col_solve": ["out"],
}
for _s in SUFFIX.values():
    SIG["hadi_compute_base_prices" + _s] = _PRICE
    SIG["hadi_compute_jacobian" + _s] = _JAC
ARGS = {"S_0": S_0, "V_0": V_0, "eps": EPS, "snap": SNAP, "n_snap": 2, "step": 2, "ex": [2, 4], "n_ex": 2, "ex_rows": 1,
        "samples": {"n_samp": 3, "spots": SPOTS[1], "scales": None, "rows": 1},
        "barrier": {"lower_i": [60.0] * 3, "upper_i": [150.0] * 3, "rebate_i": None, "n_mon": 2, "mon_steps": [1, 3], "mon_rows": 1},
        "out": 1, "J": 1, "base": 1, "greeks": 1, "lad": 1}


def _refusal_cases():
    out = []

    def add(name, fn="hadi_DO_timestepping", prob=None, args=None, **kw):
        out.append(dict(name="x_" + name, kind="refusal", fn=fn, prob=prob or {}, args=args or {}, **kw))

    DO, PDS, BP, JAC, GK = "hadi_DO_timestepping", "hadi_parallel_DO_solve", "hadi_compute_base_prices", "hadi_compute_jacobian", "hadi_compute_greeks"
    LAD, BPL, JL = "hadi_maturity_ladder", "hadi_compute_base_prices_ladder", "hadi_compute_jacobian_ladder"
    SL, BPS, JS = "hadi_sample_ladder", "hadi_compute_base_prices_samples", "hadi_compute_jacobian_samples"
    BE, BPB, JB = "hadi_bermudan_timestepping", "hadi_compute_base_prices_bermudan", "hadi_compute_jacobian_bermudan"
    KO, BPK, JK = "hadi_barrier_timestepping", "hadi_compute_base_prices_barrier", "hadi_compute_jacobian_barrier"
    ROW, COL = "hadi_debug_row_pass", "hadi_debug_col_solve"
    # ---- no handle -------------------------------------------------------------------------------------------------------------------
    for fn in (DO, PDS, BP, "hadi_compute_base_prices_american", JAC, GK, LAD, JL, SL, BE, KO, BPK, ROW):
        add("null_ctx_" + fn[5:], fn, ctx=0)
    # ---- check_problem ---------------------------------------------------------------------------------------------------------------
    add("p_null", null_p=1)
    add("p_null_american_wrapper", "hadi_compute_jacobian_american", null_p=1)
    add("n_instances_0", prob={"n_instances": 0})
    add("variant_7", prob={"variant": 7})
    add("memspace_5", prob={"memspace": 5})
    add("vec_s_null", prob={"vec_s": None})
    add("delta_s_null", prob={"delta_s": None})
    add("vec_v_null", prob={"vec_v": None})
    add("vec_v_null_rebuilt_is_fine_U_null", BP, prob={"vec_v": None, "U": None})
    add("U_null", prob={"U": None})
    add("N_0", prob={"N": 0})
    add("delta_t_0", prob={"delta_t": 0.0})
    add("delta_t_nan", prob={"delta_t": "nan"})
    add("N_i_entry_0", prob={"N_i": [4, 0, 4]})
    add("delta_t_i_inf", prob={"delta_t_i": [0.25, 0.25, "inf"]})
    add("theta_negative", prob={"theta": -1.0})
    add("option_type_3", prob={"option_type": 3})
    add("put_without_strikes", prob={"option_type": 1})
    add("put_strike_negative", prob={"option_type": 1, "strike_i": [90.0, -1.0, 110.0]})
    add("put_scheme_cs", prob={"option_type": 1, "strike_i": STRIKES, "scheme": 1})
    add("v0i_on_callers_grids", prob={"V_0_i": [0.04, 0.05, 0.06]})
    add("grid_m1_1", prob={"m1": 1})
    add("grid_m2_2", prob={"m2": 2})
    add("dividend_arrays_missing", prob={"variant": 2, "num_dividends": 2})
    add("num_dividends_negative", prob={"num_dividends": -1})
    add("scheme_9", prob={"scheme": 9})
    add("scheme_mcs_american", prob={"scheme": 2, "variant": 1})
    add("scheme_mcs_theta_0", prob={"scheme": 2, "theta": 0.0})
    add("state_precision_2", prob={"state_precision": 2})
    add("fp32_american", prob={"state_precision": 1, "variant": 1})
    add("fp32_scheme_cs", prob={"state_precision": 1, "scheme": 1})
    add("jacobian_variant_7", JAC, prob={"variant": 7})
    add("greeks_vec_v_null", GK, prob={"vec_v": None})
    # ---- the wrappers' own checks ------------------------------------------------------------------------------------------------------
    add("pds_base_null", PDS, args={"out": None})
    add("bp_base_null", BP, args={"out": None})
    add("bp_dividends_base_null", "hadi_compute_base_prices_dividends", args={"out": None})
    add("bp_bermudan_base_null", BPB, args={"out": None})
    add("barrier_null", KO, args={"barrier": None})
    add("bp_barrier_null", BPK, args={"barrier": None})
    add("bp_barrier_base_null", BPK, args={"out": None})
    add("jac_barrier_null", JK, args={"barrier": None})
    for fn in (LAD, BPL, JL, SL, BPS, JS):
        add("n_snap_0_" + fn[5:], fn, args={"n_snap": 0})
        add("snap_null_" + fn[5:], fn, args={"snap": None})
    # ---- check_ladder ------------------------------------------------------------------------------------------------------------------
    add("ladder_out_null", LAD, args={"out": None})
    add("bp_ladder_out_null", BPL, args={"out": None})
    add("jac_ladder_J_null", JL, args={"J": None})
    add("jac_ladder_base_null", JL, args={"base": None})
    add("ladder_N_i", LAD, prob={"N_i": [4, 4, 4]})
    add("ladder_n_snap_beyond_N", LAD, args={"n_snap": 5, "snap": [1, 2, 3, 4, 5]})
    add("ladder_steps_equal", LAD, args={"snap": [2, 2]})
    add("ladder_step_0", BPL, args={"snap": [0, 2]})
    add("ladder_step_beyond_N", JL, args={"snap": [2, 5]})
    add("ladder_fp32", LAD, prob={"state_precision": 1})
    add("ladder_call_r_f", LAD, prob={"r_f": 0.01})
    add("jac_ladder_call_r_f", JL, prob={"r_f": 0.01})
    # ---- check_samples -----------------------------------------------------------------------------------------------------------------
    add("samples_null", SL, args={"samples": None})
    add("samples_null_bp", BPS, args={"samples": None})
    add("samples_null_jac", JS, args={"samples": None})
    add("samples_spots_null", SL, args={"samples": {"spots": None}})
    add("samples_n_samp_0", SL, args={"samples": {"n_samp": 0}})
    add("samples_n_samp_1025", BPS, args={"samples": {"n_samp": 1025}})
    add("samples_rows_2", JS, args={"samples": {"rows": 2}})
    add("samples_scale_inf", SL, args={"samples": {"scales": [1.0, "inf", 1.0]}})
    add("samples_out_null", SL, args={"out": None})
    add("samples_fp32", SL, prob={"state_precision": 1})
    # ---- check_bermudan ----------------------------------------------------------------------------------------------------------------
    add("bermudan_american", BE, prob={"variant": 1})
    add("bermudan_american_dividends_jac", JB, prob={"variant": 3, "num_dividends": 0})
    add("bermudan_fp32", BE, prob={"state_precision": 1})
    add("bermudan_n_ex_negative", BE, args={"n_ex": -1})
    add("bermudan_rows_2", BPB, args={"ex_rows": 2})
    add("bermudan_steps_null", BE, args={"ex": None})
    add("bermudan_nonzero_behind_zero", BE, args={"n_ex": 3, "ex": [1, 0, 2]})
    add("bermudan_not_increasing", JB, args={"ex": [2, 1]})
    add("bermudan_beyond_N", BE, args={"ex": [2, 5]})
    add("bermudan_shared_beyond_min_N_i", BE, prob={"N_i": [4, 3, 4]}, args={"ex": [2, 4]})
    add("bermudan_row_1_beyond_its_N_i", BE, prob={"N_i": [4, 3, 4]}, args={"ex": [1, 2, 1, 4, 1, 2], "ex_rows": 3})
    # ---- check_barrier -----------------------------------------------------------------------------------------------------------------
    add("barrier_american", KO, prob={"variant": 1})
    add("barrier_fp32", BPK, prob={"state_precision": 1})
    add("barrier_nan", KO, args={"barrier": {"upper_i": [150.0, "nan", 150.0]}})
    add("barrier_lower_not_below_upper", JK, args={"barrier": {"lower_i": [60.0, 60.0, 150.0]}})
    add("barrier_rebate_inf", KO, args={"barrier": {"rebate_i": [0.0, 0.0, "inf"]}})
    add("barrier_monitoring_without_barrier", KO, args={"barrier": {"lower_i": None, "upper_i": None}})
    add("barrier_mon_steps_not_increasing", KO, args={"barrier": {"mon_steps": [3, 1]}})
    add("barrier_mon_steps_null", BPK, args={"barrier": {"mon_steps": None}})
    add("barrier_mon_rows_2", JK, args={"barrier": {"mon_rows": 2}})
    add("barrier_n_mon_negative", KO, args={"barrier": {"n_mon": -1}})
    # ---- the diagnostics ---------------------------------------------------------------------------------------------------------------
    add("debug_row_out_null", ROW, args={"out": None})
    add("debug_col_out_null", COL, args={"out": None})
    add("debug_row_scheme_cs", ROW, prob={"scheme": 1})
    add("debug_col_fp32", COL, prob={"state_precision": 1})
    add("debug_col_american", COL, prob={"variant": 1})
    add("debug_row_step_0", ROW, args={"step": 0})
    add("debug_row_step_beyond_N", ROW, args={"step": 5})
    # ---- the drivers' own checks -------------------------------------------------------------------------------------------------------
    add("bp_v0i_host_vgrid", BP, prob={"V_0_i": [0.04, 0.05, 0.06]}, tuning={"device_vgrid": 0})
    add("jac_v0i_host_vgrid", JAC, prob={"V_0_i": [0.04, 0.05, 0.06]}, tuning={"device_vgrid": 0})
    add("jac_U_0_null", JAC, prob={"U_0": None})
    add("jac_J_null", JAC, args={"J": None})
    add("jac_base_null", JAC, args={"base": None})
    add("jac_bermudan_J_null", JB, args={"J": None})
    add("jac_samples_base_null", JS, args={"base": None})
    add("greeks_null", GK, args={"greeks": None})
    add("greeks_fp32", GK, prob={"state_precision": 1})
    # ---- behind the sweep --------------------------------------------------------------------------------------------------------------
    add("S_0_off_pds", PDS, args={"S_0": 101.5})
    add("S_0_off_bp", BP, args={"S_0": 101.5})
    add("S_0_off_ladder", LAD, args={"S_0": 101.5})
    add("S_0_off_jac", JAC, args={"S_0": 101.5})
    add("S_0_off_jac_ladder", JL, args={"S_0": 101.5})
    add("S_0_off_greeks", GK, args={"S_0": 101.5})
    add("V_0_off_greeks", GK, args={"V_0": 0.0412345})
    add("sample_off_grid", SL, args={"samples": {"spots": [80.0, 1e9, 100.0]}})
    add("sample_off_grid_jac", JS, args={"samples": {"spots": [80.0, 100.0, -1.0]}})
    add("sample_degenerate", SL, grid="small_deg", args={"samples": {"spots": [80.0, "deg", 100.0]}})
    add("sample_degenerate_and_off_grid", BPS, grid="small_deg", args={"samples": {"spots": [1e9, "deg", 100.0]}})
    # ---- two violations at once: the winner is the order of the checks -----------------------------------------------------------------
    add("both_base_null_and_p_null", BP, null_p=1, args={"out": None})
    add("both_barrier_null_and_base_null", BPK, args={"barrier": None, "out": None})
    add("both_bermudan_american_and_fp32", BE, prob={"variant": 1, "state_precision": 1})
    add("both_ladder_n_snap_0_and_N_i", LAD, prob={"N_i": [4, 4, 4]}, args={"n_snap": 0})
    add("both_samples_null_and_bad_snap_steps", SL, args={"samples": None, "snap": [4, 2]})
    add("both_jac_ladder_U_0_null_and_J_null", JL, prob={"U_0": None}, args={"J": None})
    add("both_barrier_nan_and_bad_mon_steps", KO, args={"barrier": {"lower_i": [60.0, "nan", 60.0], "mon_steps": [3, 1]}})
    add("both_bermudan_base_null_and_bad_schedule", BPB, args={"ex": [2, 1], "out": None})
    add("both_jac_U_0_null_and_v0i_host_vgrid", JAC, prob={"U_0": None, "V_0_i": [0.04, 0.05, 0.06]}, tuning={"device_vgrid": 0})
    add("both_debug_out_null_and_bad_step", ROW, args={"out": None, "step": 9})
    return out


CASES = _result_cases() + _refusal_cases()


def filled(case):
    return {**DEFAULTS, **case} if case.get("kind", "result") == "result" else case


def _sha(x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _env(H, grid):
    m1, m2, tuning = GRIDS["small" if grid == "small_deg" else grid]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, STRIKES)
    deg = None
    if grid == "small_deg":  # instance 0: two equal s-nodes; `deg` lies in the interval behind them
        grids.Vec_s[0, 31] = grids.Vec_s[0, 30]
        deg = 0.5 * (grids.Vec_s[0, 31] + grids.Vec_s[0, 32])
    return m1, m2, tuning, grids, deg


def _once(H, sv, c):
    """One call of a result case: the list of arrays it returns or writes."""
    m1, m2, _, grids, _ = _env(H, c["grid"])
    n, m, N, dt = len(STRIKES), (m1 + 1) * (m2 + 1), N_STEPS, T / N_STEPS
    dev = c["mem"] == "device"
    if dev:
        import torch
        where = torch.device("cuda", sv.device_id)
        grids_h, grids = grids, grids.to(where)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(where)
    else:
        grids_h, put = grids, lambda a: np.ascontiguousarray(a).copy()
    U0h = grids_h.put_payoff(STRIKES) if c["put"] else grids_h.call_payoff(STRIKES)
    variant, call = VARIANTS[c["variant"]], c["call"]
    am, div = variant in (1, 3), variant in (2, 3)
    dividends = H.Dividends(*DIVS) if div else None
    per = {}
    if c["v0i"]:
        per["V_0_i"] = [0.04, 0.05, 0.06]
    if c["dti"]:
        per["delta_t_i"] = [0.25, 0.2, 0.3]
    opt = dict(option_type=H.PUT, strikes=STRIKES) if c["put"] else {}
    if c["put"] and call not in ("do", "greeks", "ladder", "sample", "berm", "barrier", "dbg_row"):
        per.update(opt)  # (the launchers carry the put in per_instance)
    per = per or None
    head = (m1, m2, N, dt, THETA, R_D, c["r_f"], RHO, SIGMA, KAPPA, ETA)
    lhead = (R_D, c["r_f"], RHO, SIGMA, KAPPA, ETA, m1, m2, m, N, THETA, dt, n, grids)  # the launchers' middle
    U = put(U0h)
    U_0 = put(U0h) if am else None
    kw = dict(variant=variant, dividends=dividends, per_instance=per)
    rows = c["rows"]

    def ws():
        w = H.DOWorkspace(n, m, where if dev else None)
        w.U[...] = put(U0h)
        return w

    if call == "do":
        lam = put(np.zeros_like(U0h)) if am else None
        sv.DO_timestepping(*head, grids, U, U_0=U_0, lambda_bar=lam, **kw, **opt)
        return [U] + ([lam] if am else [])
    if call == "pds":
        w = ws()
        return [sv.parallel_DO_solve(n, S_0, V_0, *head[:3], T, *head[3:], grids, w), w.U]
    if call == "bp":
        w = ws()
        tail = ([U_0] if am else []) + [w] + ([dividends] if div else [])
        return [getattr(sv, "compute_base_prices" + SUFFIX[c["variant"]])(S_0, V_0, T, *lhead, *tail, per_instance=per), w.U]
    if call == "jac":
        tail = [put(U0h)] + ([dividends] if div else [])
        return list(getattr(sv, "compute_jacobian" + SUFFIX[c["variant"]])(S_0, V_0, T, *lhead, *tail, eps=EPS, per_instance=per))
    if call == "greeks":
        res = sv.compute_greeks(*head, grids, U, S_0, V_0, U_0=U_0, ladder=bool(c["lad"]), **kw, **opt)
        return list(res) if c["lad"] else [res]
    if call == "dbg_row":
        return [sv.debug_row_pass(*head, grids, U, step=2, variant=variant, U_0=U_0, **opt)]
    if call == "dbg_col":
        return [sv.debug_col_solve(*head, grids, U)]
    # the four features: what the call carries behind the state (positional), and by keyword
    fam, feat = ("", call) if "_" not in call else call.split("_")
    feat = {"samples": "sample"}.get(feat, feat)
    extra = {"ladder": (SNAP,), "sample": (SNAP,), "berm": (SCHED[rows],), "barrier": (SCHED[rows],)}[feat]
    if feat == "sample":
        kw["scales"] = SCALES[rows]
    if feat == "barrier":
        kw.update(BARRIER)
    elif fam != "jac":
        kw["U_0"] = U_0
    lead = (SPOTS[rows], V_0) if feat == "sample" else (S_0, V_0)
    if not fam:  # on the caller's grids
        name = {"ladder": "maturity_ladder", "sample": "sample_ladder", "berm": "bermudan_timestepping", "barrier": "barrier_timestepping"}[feat]
        return [getattr(sv, name)(*head, grids, U, *(lead if feat in ("ladder", "sample") else ()), *extra, **kw, **opt)]
    name = ("compute_base_prices_" if fam == "bp" else "compute_jacobian_") + {"berm": "bermudan", "sample": "samples"}.get(feat, feat)
    if fam == "jac":
        return list(getattr(sv, name)(*lead, *lhead, put(U0h), *extra, eps=EPS, **kw))
    w = ws()
    return [getattr(sv, name)(*lead, *lhead, w, *extra, **kw)] + ([w.U] if feat in ("berm", "barrier") else [])


def _run_result(H, case, lib_path):
    c = filled(case)
    tuning = dict(GRIDS[c["grid"]][2])
    if c["dv"] is not None:
        tuning["device_vgrid"] = c["dv"]
    with H.HestonADI(0, lib_path=lib_path) as sv:
        for k, v in tuning.items():
            sv.set_tuning(k, v)
        before = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
        res = [[_sha(x) for x in _once(H, sv, c)] for _ in range(2)]
        desc = sv.describe_last_sweep()
        after = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
    assert res[0] == res[1], "%s: two identical calls on one handle returned different bytes" % c["name"]
    return {"desc": desc, "graph": [after[0] - before[0], after[1] - before[1]], "sha256": res[1]}


def _f64(v, deg=None):
    return np.array([deg if x == "deg" else float(x) for x in v], dtype=np.float64)


def _run_refusal(H, c, lib_path):
    from pde_based_heston_solver_gpu_accelerated_amd import _native as nat
    m1, m2, tuning, grids, deg = _env(H, c.get("grid", "small"))
    tuning = {**tuning, **c.get("tuning", {})}
    n, m, dt = len(STRIKES), (m1 + 1) * (m2 + 1), T / N_STEPS
    keep = []
    dp = lambda a: (keep.append(a), a.ctypes.data_as(nat._dp))[1]
    ip = lambda v: (keep.append(np.array(v, dtype=np.int32)), keep[-1].ctypes.data_as(nat._ip))[1]
    buf = lambda: (keep.append(np.zeros(n * m * 8)), C.c_void_p(keep[-1].ctypes.data))[1]
    U0 = grids.call_payoff(STRIKES)
    with H.HestonADI(0, lib_path=lib_path) as sv:
        for k, v in tuning.items():
            sv.set_tuning(k, v)
        p = sv._problem(0, m1, m2, N_STEPS, dt, THETA, R_D, 0.0, RHO, SIGMA, KAPPA, ETA, grids, U=U0.copy(), U_0=U0.copy())
        for k, v in c["prob"].items():
            if k == "N_i":
                v = ip(v)
            elif isinstance(v, list):
                v = dp(_f64(v))
            elif isinstance(v, str):
                v = float(v)
            setattr(p, k, v)
        a = {**ARGS, **{k: v for k, v in c["args"].items() if k not in ("samples", "barrier")}}
        for k in ("samples", "barrier"):  # a dict overrides fields of the default struct, None is the NULL struct
            a[k] = None if c["args"].get(k, 0) is None else {**ARGS[k], **c["args"].get(k, {})}
        argv = []
        for tok in SIG[c["fn"]]:
            v = a[tok]
            if tok in ("out", "J", "base", "greeks", "lad"):
                v = buf() if v else None
            elif tok in ("snap", "ex"):
                v = ip(v) if v is not None else None
            elif tok == "samples" and v is not None:
                s = v
                v = C.byref(nat.Samples(s["n_samp"], dp(_f64(s["spots"], deg)) if s["spots"] is not None else None,
                                        dp(_f64(s["scales"])) if s["scales"] is not None else None, s["rows"]))
            elif tok == "barrier" and v is not None:
                b = v
                arr = lambda x: dp(_f64(x)) if x is not None else None
                v = C.byref(nat.Barrier(arr(b["lower_i"]), arr(b["upper_i"]), arr(b["rebate_i"]), b["n_mon"],
                                        ip(b["mon_steps"]) if b["mon_steps"] is not None else None, b["mon_rows"]))
            argv.append(v)
        h = sv._h if c.get("ctx", 1) else None
        rc = getattr(sv._lib, c["fn"])(h, None if c.get("null_p") else C.byref(p), *argv)
        msg = sv._lib.hadi_last_error(h).decode()
    return {"status": rc, "message": msg}


def run_case(H, case, lib_path=None):
    return (_run_refusal if case.get("kind") == "refusal" else _run_result)(H, case, lib_path)


def compare(recorded, got):
    """What the replay of a fixture case must reproduce, exactly; returns the list of differences (empty: none)."""
    return ["%s: recorded %r, now %r" % (k, recorded[k], got[k]) for k in got if recorded[k] != got[k]]


def holds(H, case, got, lib_path=None):
    """A result case walks the code path it is there for -- a dividend case pays one: no array it returns has the bytes of the same
    call without dividends; a refusal case is refused."""
    if case.get("kind") == "refusal":
        return got["status"] != 0
    c = filled(case)
    if c["variant"] in NO_DIVIDENDS:
        twin = run_case(H, {**case, "variant": NO_DIVIDENDS[c["variant"]]}, lib_path)
        if any(a == b for a, b in zip(got["sha256"], twin["sha256"])):
            return False
    return case.get("expect", EXPECT[c["grid"]]) in got["desc"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libhadi.so (same ABI)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--check", action="store_true", help="replay the fixture instead of recording it")
    ap.add_argument("--against", default=None, help="a first recording of the same build: every case must agree")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pde_based_heston_solver_gpu_accelerated_amd as H
    if a.check:
        fix = json.load(open(FIXTURE))
        bad = 0
        for rec in fix["cases"]:
            diff = compare(rec, run_case(H, rec["in"], a.lib))
            bad += bool(diff)
            print("%-48s %s" % (rec["in"]["name"], "ok" if not diff else "; ".join(diff)), flush=True)
        print("%d of %d cases differ" % (bad, len(fix["cases"])))
        return 1 if bad else 0
    first = {r["in"]["name"]: r for r in json.load(open(a.against))["cases"]} if a.against else {}
    rows, bad = [], 0
    for case in CASES:
        try:
            got = run_case(H, case, a.lib)
        except (TypeError, ValueError, KeyError, AttributeError, H.HadiError) as e:  # a mistake in the case list: name it, go on
            if getattr(e, "status", 1) not in (1, 2, 4):
                raise
            print("%-48s NOT RECORDED: %r" % (case["name"], e), flush=True)
            bad += 1
            continue
        ok = holds(H, case, got, a.lib)
        same = not first or not compare(first[case["name"]], got)
        bad += not (ok and same)
        print("%-48s %s%s%s" % (case["name"], "" if ok else "MISSES ITS BRANCH ", "" if same else "DIFFERS FROM THE FIRST RECORDING ",
                                json.dumps(got)), flush=True)
        rows.append({"in": case, **got})
    with open(a.out, "w") as f:
        f.write('{"defaults": %s,\n "cases": [\n' % json.dumps(DEFAULTS))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print("%d cases -> %s; %d miss their branch or differ from the first recording" % (len(rows), a.out, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
