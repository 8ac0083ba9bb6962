"""Records (or, with --check, replays) tests/golden/route_selection.json: which route a whole call takes.

Every case is a small call through the public Python API only -- set_tuning, DO_timestepping / maturity_ladder,
describe_last_sweep and get_tuning of the graph counters -- on a fresh handle, twice.  Recorded per case: the inputs, the full
description, the deltas of graph_captures / graph_replays over the two calls and the SHA-256 of the returned array's bytes.

    python tools/record_routes.py [--lib other/libhadi.so] [--out file.json]   # record (the committed fixture: from the parent build)
    python tools/record_routes.py --check [--lib ...]                           # replay the committed fixture and compare

Recording twice and comparing the two files (--against first.json) shows whether every hash is a property of the build; a case
whose hash differs between two recordings of one build has no place in the fixture.  tests/test_gpu_route_selection.py runs
run_case() and compare() below, so the test and --check are one implementation.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_selection.json")
CU_COUNT = 256  # the device the fixture is recorded on (cases with "cu256" set mean nothing elsewhere)

S_0, V_0, T, R_D = 100.0, 0.04, 1.0, 0.025
RHO, SIGMA, KAPPA, ETA = -0.9, 0.3, 1.5, 0.04
DIVS = ([0.2, 0.4, 0.6, 0.8], [0.5, 0.3, 0.2, 0.1], [0.02] * 4)
# what a case may leave out
DEFAULTS = {"call": "solve", "variant": "EU", "scheme": 0, "prec": 0, "theta": 0.8, "r_f": 0.01, "steps": 2, "tuning": {},
            "profiling": 0, "payoff": "s", "snap": [1, 2], "cu256": 1}
VARIANTS = {"EU": 0, "AM": 1, "DIV": 2, "AM_DIV": 3}
MCS, HV, CS = 2, 3, 1


def _cases():
    out = []

    def add(name, m1, m2, n, expect, **kw):
        """expect: a piece of text the description must hold (the branch the case is there for; '!x': must not hold x)."""
        out.append(dict(name=name, m1=m1, m2=m2, n=n, expect=expect, **kw))

    SCH, SMALL, SEQ, SEQ2 = "hadi_small_sch_kernel", "hadi_small_kernel", "hadi_small_seq_kernel", "hadi_small_seq2_kernel"
    TEAM, RES = "hadi_team_kernel", "hadi_sweep_resident<8>"
    # ---- predictor-corrector sweeps of small grids in LDS --------------------------------------------------------------
    add("sch_auto_257", 50, 25, 257, SCH + "<1,MCS>", scheme=MCS)
    add("sch_auto_256_streams", 50, 25, 256, "!" + SCH, scheme=MCS)
    add("sch_forced_4", 50, 25, 4, SCH, scheme=MCS, tuning={"small_sch": 1}, cu256=0)
    add("sch_never_257", 50, 25, 257, "!" + SCH, scheme=MCS, tuning={"small_sch": 0})
    add("sch_100x30_500_streams", 100, 30, 500, "!" + SCH, scheme=MCS)
    add("sch_100x30_forced_500", 100, 30, 500, SCH, scheme=MCS, tuning={"small_sch": 1}, cu256=0)
    add("sch_strip_pinned_257", 50, 25, 257, "!" + SCH, scheme=MCS, tuning={"strip": 0})
    add("sch_cs_strips0_257", 50, 25, 257, "!" + SCH, scheme=MCS, tuning={"cs_strips": 0})
    add("sch_profiling_257", 50, 25, 257, "!" + SCH, scheme=MCS, profiling=1)
    add("sch_hv_257", 50, 25, 257, SCH + "<1,HV>", scheme=HV)
    add("sch_cs_257", 50, 25, 257, SCH + "<1,CS>", scheme=CS)
    add("sch_small_grid0_257", 50, 25, 257, "!" + SCH, scheme=MCS, tuning={"small_grid": 0})
    # ---- the small block kernel and its one-wavefront variants -------------------------------------------------------------
    add("small_4", 50, 25, 4, SMALL + "<1,8,EU>")
    add("small_256", 50, 25, 256, SMALL + "<1,8,EU>")
    add("small_seq_257", 50, 25, 257, SEQ + "<1>")
    add("small_w8_512", 50, 25, 512, SMALL + "<1,8,EU>", tuning={"small_seq": 0})
    add("small_w4_513", 50, 25, 513, SMALL + "<1,4,EU>", tuning={"small_seq": 0})
    add("small_seq_512", 50, 25, 512, SEQ + "<1>")
    add("small_seq2_513", 50, 25, 513, SEQ2 + "<1>")
    add("small_seq2_1152", 50, 25, 1152, SEQ2 + "<1>")
    add("small_seq_1153", 50, 25, 1153, SEQ + "<1>")
    add("small_seq_forced_4", 50, 25, 4, SEQ + "<1>", tuning={"small_seq": 1}, cu256=0)
    add("small_pairs_forced_4", 50, 25, 4, SEQ2 + "<1>", tuning={"small_seq": 1, "small_pairs": 1}, cu256=0)
    add("small_pairs_never_600", 50, 25, 600, SEQ + "<1>", tuning={"small_pairs": 0})
    add("small_waves4_4", 50, 25, 4, SMALL + "<1,4,EU>", tuning={"small_waves": 4}, cu256=0)
    add("small_am_4", 50, 25, 4, SMALL + "<1,8,AM>", variant="AM")
    add("small_am_300", 50, 25, 300, SMALL + "<1,8,AM>", variant="AM")
    add("small_am_600", 50, 25, 600, SMALL + "<1,4,AM>", variant="AM")
    add("small_div_4", 50, 25, 4, SMALL + "<1,8,EU>", variant="DIV")
    add("small_div_seq_257", 50, 25, 257, SEQ + "<1>", variant="DIV")
    add("small_grid0_4", 50, 25, 4, "row pass hadi_pass_a<", tuning={"small_grid": 0})
    add("small_fp32_4", 50, 25, 4, "row pass hadi_pass_a<", prec=1)
    add("small_profiling_4", 50, 25, 4, "row pass hadi_pass_a<", profiling=1)
    add("small_ladder_4", 50, 25, 4, "snapshots copied inside the time loop", call="ladder", r_f=0.0)
    # ---- instance-resident launch (the team) ---------------------------------------------------------------------------------
    add("team_1", 300, 80, 1, TEAM + "<8>")
    add("team_8", 300, 80, 8, TEAM + "<8>")
    add("team_9_streams", 300, 80, 9, "!" + TEAM)
    add("team_div_2", 300, 80, 2, TEAM + "<8>", variant="DIV")
    add("team_b4_2", 200, 60, 2, TEAM + "<4>")
    add("team_pinned_2", 300, 80, 2, "!" + TEAM, tuning={"strip": 1})
    add("team_pinned_forced_2", 300, 80, 2, TEAM, tuning={"strip": 1, "team_launch": 1})
    add("team_never_2", 300, 80, 2, "!" + TEAM, tuning={"team_launch": 0})
    add("team_theta0_2", 300, 80, 2, "!" + TEAM, theta=0.0)
    add("team_rd_eq_rf_2", 300, 80, 2, "!" + TEAM, r_f=R_D)
    add("team_ladder_2", 300, 80, 2, "hadi_snap_kernel after each snapshot step", call="ladder", r_f=0.0)
    add("team_am_2", 300, 80, 2, "!" + TEAM, variant="AM")
    # ---- resident sweep ------------------------------------------------------------------------------------------------------
    add("resident_246", 300, 80, 246, RES)
    add("resident_256", 300, 80, 256, RES)
    add("resident_245_streams", 300, 80, 245, "!" + RES)
    add("resident_257_streams", 300, 80, 257, "!" + RES)
    add("resident_never_256", 300, 80, 256, "!" + RES, tuning={"resident_sweep": 0})
    add("resident_pinned_256", 300, 80, 256, "!" + RES, tuning={"strip": 1})
    add("resident_pinned_forced_256", 300, 80, 256, RES, tuning={"strip": 1, "resident_sweep": 1})
    add("resident_debug_fault_256", 300, 80, 256, "!" + RES, tuning={"debug_fault": 256, "resident_sweep": 1})
    add("resident_ladder_256", 300, 80, 256, "!" + RES, call="ladder", r_f=0.0)
    add("resident_profiling_256", 300, 80, 256, "!" + RES, profiling=1)
    add("resident_am_256", 300, 80, 256, "!" + RES, variant="AM")
    # ---- sub-batches: a round of 256 instances of 512x128 streams 256 MiB and more ----------------------------------------------
    add("sub_320", 512, 128, 320, "2 sub-batches of 256 64 instances")
    add("sub_300_rides_along", 512, 128, 300, "!of 256")
    add("sub_batch0_320", 512, 128, 320, "!of 256", tuning={"sub_batch": 0})
    add("sub_320_one_stream", 512, 128, 320, "!two streams", tuning={"streams": 1})
    add("sub_320_streaming", 512, 128, 320, "!" + RES, tuning={"resident_sweep": 0})
    add("sub_384_alternate", 512, 128, 384, "2 sub-batches of 256 128 instances (each with the geometry of its own size), side by side on two streams")
    add("sub_384_streaming_alternate", 512, 128, 384, "side by side on two streams", tuning={"resident_sweep": 0})
    add("sub_384_one_stream", 512, 128, 384, "!two streams", tuning={"streams": 1})
    add("sub_500_last_two", 512, 128, 500, "3 sub-batches of 256 122 122 instances (each with the geometry of its own size), the last two side by side")
    add("sub_502_both_resident", 512, 128, 502, "in one launch: " + RES)
    # ---- two streams -----------------------------------------------------------------------------------------------------------
    add("streams_auto_half_cut_160", 512, 256, 160, "2 sub-batches of 80 instances, side by side on two streams")
    add("streams_pinned_half_cut_160", 300, 80, 160, "2 sub-batches of 80 instances, side by side on two streams", tuning={"strip": 1})
    add("streams_ring_160_one", 300, 80, 160, "!two streams")
    add("streams_forced_2_64", 300, 80, 64, "side by side on two streams", tuning={"streams": 2})
    add("streams_forced_1_160", 300, 80, 160, "!two streams", tuning={"streams": 1})
    add("streams_cs_160_one", 300, 80, 160, "!two streams", scheme=CS)
    # ---- American sweeps in the P representation ----------------------------------------------------------------------------
    add("amp_s_only_16", 300, 80, 16, "AM-P", variant="AM")
    add("amp_v_payoff_16", 300, 80, 16, "!AM-P", variant="AM", payoff="sv")
    add("amp_off_16", 300, 80, 16, "!AM-P", variant="AM", tuning={"american_p": 0})
    add("amp_ladder_16", 300, 80, 16, "!AM-P", variant="AM", call="ladder", r_f=0.0)
    add("amp_div_16", 300, 80, 16, "AM-P", variant="AM_DIV")
    # ---- shapes beyond the streaming kernels: sequential passes ---------------------------------------------------------------
    add("row_seq_1100x20", 1100, 20, 2, "hadi_pass_a_seq")
    add("col_seq_40x600", 40, 600, 2, "hadi_pass_b_seq")
    # ---- graph replay ------------------------------------------------------------------------------------------------------------
    add("graph_on_16", 300, 80, 16, "row pass")
    add("graph_off_16", 300, 80, 16, "row pass", tuning={"graph": 0})
    add("graph_max_melems_within_16", 300, 80, 16, "row pass", tuning={"graph_max_melems": 1})
    add("graph_max_melems_beyond_32", 300, 80, 32, "row pass", tuning={"graph_max_melems": 1})
    # ---- the rest of what the streaming description words -----------------------------------------------------------------------
    add("stream_fp32_16", 300, 80, 16, "float", prec=1)
    add("stream_cs_16", 300, 80, 16, "CS", scheme=CS)
    add("stream_div_16", 300, 80, 16, "row pass", variant="DIV")
    add("stream_hv_100x30_16", 100, 30, 16, "HV", scheme=HV)
    return out


CASES = _cases()


def filled(case):
    return {**DEFAULTS, **case}


def run_case(H, case, lib_path=None):
    """The case twice on a fresh handle: {"desc", "graph": [captures, replays], "sha256"} -- and the two results must be the
    same bytes."""
    c = filled(case)
    m1, m2, n, N = c["m1"], c["m2"], c["n"], c["steps"]
    strikes = [100.0] if n == 1 else [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    U0 = grids.call_payoff(strikes)
    if c["payoff"] == "sv":  # a payoff that depends on v: the explicit (U, lambda_bar) representation
        U0 = np.ascontiguousarray((U0.reshape(n, m2 + 1, m1 + 1) + 0.5 * grids.Vec_v[:, :, None]).reshape(n, -1))
    variant = VARIANTS[c["variant"]]
    kw = dict(variant=variant, scheme=c["scheme"])
    if variant in (1, 3):
        kw["U_0"] = U0
    if variant in (2, 3):
        kw["dividends"] = H.Dividends(*DIVS)
    args = (m1, m2, N, T / N, c["theta"], R_D, c["r_f"], RHO, SIGMA, KAPPA, ETA, grids)
    with H.HestonADI(0, lib_path=lib_path) as sv:
        for k, v in c["tuning"].items():
            sv.set_tuning(k, v)
        sv.set_profiling(bool(c["profiling"]))
        before = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
        res = []
        for _ in range(2):
            U = U0.copy()
            if c["call"] == "ladder":
                out = sv.maturity_ladder(*args, U, S_0, V_0, c["snap"], **kw)
            else:
                lam = np.zeros_like(U) if variant in (1, 3) else None
                out = sv.DO_timestepping(*args, U, state_precision=c["prec"], lambda_bar=lam, **kw)
            res.append(hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest())
        desc = sv.describe_last_sweep()
        after = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
        cus = sv.device_info()["compute_units"]
    assert res[0] == res[1], "%s: two identical calls on one handle returned different bytes" % c["name"]
    return {"desc": desc, "graph": [after[0] - before[0], after[1] - before[1]], "sha256": res[1], "cu_count": cus}


def holds(expect, desc):
    return expect[1:] not in desc if expect.startswith("!") else expect in desc


def compare(recorded, got):
    """What the replay of a fixture case must reproduce, exactly; returns the list of differences (empty: none)."""
    return ["%s: recorded %r, now %r" % (k, recorded[k], got[k]) for k in ("desc", "graph", "sha256") if recorded[k] != got[k]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libhadi.so (same ABI)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--check", action="store_true", help="replay the fixture instead of recording it")
    ap.add_argument("--against", default=None, help="a first recording of the same build: every hash must agree")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pde_based_heston_solver_gpu_accelerated_amd as H
    if a.check:
        fix = json.load(open(FIXTURE))
        bad = 0
        for rec in fix["cases"]:
            got = run_case(H, rec["in"], a.lib)
            if rec["in"].get("cu256", 1) and got["cu_count"] != fix["cu_count"]:
                print("%-32s skipped (recorded on %d CUs)" % (rec["in"]["name"], fix["cu_count"]))
                continue
            diff = compare(rec, got)
            bad += bool(diff)
            print("%-32s %s" % (rec["in"]["name"], "ok" if not diff else "; ".join(diff)), flush=True)
        print("%d of %d cases differ" % (bad, len(fix["cases"])))
        return 1 if bad else 0
    first = {r["in"]["name"]: r for r in json.load(open(a.against))["cases"]} if a.against else {}
    rows, bad = [], 0
    for case in CASES:
        got = run_case(H, case, a.lib)
        assert got.pop("cu_count") == CU_COUNT, "the fixture is recorded on the %d-CU device" % CU_COUNT
        ok = holds(case["expect"], got["desc"])
        same = not first or not compare(first[case["name"]], got)
        bad += not (ok and same)
        print("%-32s %s%s %s %s" % (case["name"], "" if ok else "MISSES ITS BRANCH ", "" if same else "DIFFERS FROM THE FIRST RECORDING ",
                                    got["graph"], got["desc"]), flush=True)
        rows.append({"in": case, **got})
    with open(a.out, "w") as f:
        f.write('{"cu_count": %d,\n "defaults": %s,\n "cases": [\n' % (CU_COUNT, json.dumps(DEFAULTS)))
        f.write(",\n".join("  {\"in\": %s,\n   \"graph\": %s, \"sha256\": \"%s\",\n   \"desc\": %s}"
                           % (json.dumps(r["in"]), json.dumps(r["graph"]), r["sha256"], json.dumps(r["desc"])) for r in rows))
        f.write("\n ]}\n")
    print("%d cases -> %s; %d miss their branch or differ from the first recording" % (len(rows), a.out, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
