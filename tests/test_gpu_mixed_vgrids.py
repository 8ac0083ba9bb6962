"""Every kernel family and launcher on batches whose instances carry DIFFERENT v-grids.

hadi_problem.vec_v / delta_v are [n][m2+1] / [n][m2], and the library leans on that: the Jacobian's sixth group is rebuilt on
the device for V_0 + eps, V_0_i rebuilds every instance's grid.  Every table derived from the v-grid (rowc, pb, rinv, a2i,
b2row, the paired strips' rs_tab, the team kernel's RT, the resident sweep's staged invariants, the tables of the
two-instances-per-wavefront kernel) is addressed by instance.  The rest of the suite builds its batches with
GridViewsBatch.for_strikes -- one v-grid for the whole batch -- so a kernel reading instance 0's, a neighbour's or a
sub-batch's first table would pass it.  Here neighbours never share a v-grid (Cm.mixed_vgrid_batch; a wrong-instance read is
worth 1e-3 .. 1e-2 of max|U|, tests/test_emu_mixed_vgrids.py::test_a_wrong_instances_v_grid_cannot_pass) and every instance
goes against the reference solved on ITS grids.

No new launch configuration: shapes and tuning keys are those of test_gpu_kernel_selection.py, test_gpu_pins.py (PUT_CASES,
two streams), test_gpu_resident.py, test_gpu_regressions.py (team kernel), test_gpu_schemes.py and test_gpu_small_sch.py.
Bounds: field 1e-10 max|U_ref| per instance (well-conditioned grids, asserted by the helper), fp32 state 2e-7 N, lambda_bar
1e-8 max(1, max|lambda|), prices 1e-9, J 2e-4.  Every case asserts from describe_last_sweep() which kernel ran and prints its
observed maximum."""
import functools
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm
import greeks_ref as G
import scheme_ref as S

pytestmark = pytest.mark.gpu

R_F = 0.01  # (the strip kernels need r_d != r_f; the b1 terms carry weight)
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
RESIDENT = "hadi_sweep_resident<8>"
SMALL_SCH = "hadi_small_sch_kernel<"
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "pair_strips": -1, "small_seq": -1,
            "small_pairs": -1, "small_sch": -1, "american_p": 1, "col_prefetch": 0, "tile_interleave": 0, "streams": 0}
OV = {H.EU: O.EU, H.AM: O.AM, H.DIV: O.DIV, H.AM_DIV: O.AM_DIV}


class _tuned:
    """Tuning keys for the block; every one goes back to its default on the way out."""

    def __init__(self, sv, tuning):
        self.sv, self.tuning = sv, tuning

    def __enter__(self):
        for k, v in self.tuning.items():
            self.sv.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.tuning:
            self.sv.set_tuning(k, DEFAULTS[k])


def _has(d, present=(), absent=()):
    for e in present:
        assert e in d, (e, d)
    for e in absent:
        assert e not in d, (e, d)


@functools.lru_cache(maxsize=None)
def _batch(m1, m2, n, put=False, same_v0=None):
    """(strikes, grids, U0, v0s) of the mixed-v-grid batch, built once per shape and size and left unchanged."""
    strikes, grids, v0s = Cm.mixed_vgrid_batch(m1, m2, n, same_v0)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0, v0s


def _sweep(sv, tuning, m1, m2, N, n, variant=H.EU, put=False, r_f=R_F, scheme=0, theta=Cm.THETA, fp32=False):
    """One DO_timestepping of the mixed batch under `tuning` -> (U_T, lambda_bar_T or None, description)."""
    strikes, grids, U0, _ = _batch(m1, m2, n, put)
    american = variant in (H.AM, H.AM_DIV)
    U, lam = U0.copy(), (np.zeros_like(U0) if american else None)
    with _tuned(sv, tuning):
        sv.DO_timestepping(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, *MODEL, grids, U, variant=variant,
                           U_0=U0.copy() if american else None, lambda_bar=lam,
                           dividends=H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None, scheme=scheme,
                           state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64, option_type=H.PUT if put else H.CALL,
                           strikes=strikes if put else None)
        d = sv.describe_last_sweep()
    return U, lam, d


@functools.lru_cache(maxsize=None)
def _reference(m1, m2, N, n, variant=H.EU, put=False, r_f=R_F, scheme=0, theta=Cm.THETA, fp32=False, rows=None):
    """Every instance (or `rows`) on its OWN grids: the oracle on 16 threads (Douglas, Craig-Sneyd), tests/scheme_ref.py
    (MCS, HV).  Computed once per case, shared and left unchanged."""
    strikes, g, U0, _ = _batch(m1, m2, n, put)
    r = np.arange(n) if rows is None else np.array(rows)
    ov = OV[variant]
    p = O.make_params(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, *MODEL, ov, Cm.DIVS if ov in (O.DIV, O.AM_DIV) else None,
                      scheme=1 if scheme == H.SCHEME_CRAIG_SNEYD else 0, state_fp32=1 if fp32 else 0,
                      option_type=O.PUT if put else O.CALL, strikes=np.asarray(strikes, dtype=np.float64)[r] if put else None)
    if scheme in (H.SCHEME_MCS, H.SCHEME_HV):
        Uo = S.solve_batch(p, g.Vec_s[r], g.Vec_v[r], g.Delta_s[r], g.Delta_v[r], U0[r], S.MCS if scheme == H.SCHEME_MCS else S.HV)
        return Uo, None
    Uo, lo, _ = O.solve_batch(p, g.Vec_s[r], g.Vec_v[r], g.Delta_s[r], g.Delta_v[r], U0[r], U0[r], threads=16, want_lambda=True)
    assert np.isfinite(Uo).all()
    return Uo, lo


def _field_errors(U, Uo):
    """Per instance: max|U - U_ref| / max|U_ref|."""
    return np.abs(U - Uo).max(axis=1) / np.abs(Uo).max(axis=1)


def _check(name, U, lam, Uo, lo, bound=1e-10):
    e = _field_errors(U, Uo)
    msg = "%s: field error %.3e of max|U_ref| (instance %d of %d)" % (name, e.max(), int(e.argmax()), len(e))
    if lam is not None:
        el = np.abs(lam - lo).max() / max(1.0, np.abs(lo).max())
        msg += ", lambda_bar %.3e" % el
    print(msg)
    assert e.max() <= bound, msg
    assert lam is None or el <= 1e-8, msg
    return float(e.max())


def _run_case(sv, name, tuning, want, m1, m2, N, n, absent=(), **kw):
    U, lam, d = _sweep(sv, tuning, m1, m2, N, n, **kw)
    _has(d, want, absent)
    Uo, lo = _reference(m1, m2, N, n, **kw)
    return _check(name, U, lam, Uo, lo, bound=2e-7 * N if kw.get("fp32") else 1e-10)


def _st(**tuning):
    return {**STREAMING, **tuning}


# ---- A. Douglas, one case per family ------------------------------------------------------------------------------------
#          id                 m1    m2   n  tuning                                        the description names         and not
FAMILIES = [
    ("small_eu",              50,   25,  4, {"small_seq": 0},                             ["hadi_small_kernel<1,", ",EU>"], [], {}),
    ("small_am",              50,   25,  4, {},                                           ["hadi_small_kernel<1,", ",AM>"], [], dict(variant=H.AM)),
    ("small_seq",             50,   25,  4, {"small_seq": 1},                             ["hadi_small_seq_kernel<1>"], [], {}),
    ("small_seq2_n5",         50,   25,  5, {"small_seq": 1, "small_pairs": 1},           ["hadi_small_seq2_kernel<1>"], [], {}),
    ("small_seq2_n7",         50,   25,  7, {"small_seq": 1, "small_pairs": 1},           ["hadi_small_seq2_kernel<1>"], [], {}),
    ("ring_b1",               50,   25,  4, _st(),                                        ["hadi_pass_a<1,1,"], ["strip"], {}),
    ("ring_b2",               128,  64,  4, _st(),                                        ["hadi_pass_a<2,1,"], ["strip"], {}),
    ("ring_b4",               200,  60,  4, _st(),                                        ["hadi_pass_a<4,1,"], ["strip"], {}),
    ("ring_b8",               300,  80,  4, _st(),                                        ["hadi_pass_a<8,1,"], ["strip"], {}),
    ("ring_two_wavefronts",   600,  40,  4, _st(),                                        ["hadi_pass_a<8,2,"], ["strip"], {}),
    ("strips_b2",             100,  50,  4, _st(strip=1),                                 ["hadi_pass_a_strip<2,EU>"], [], {}),
    ("strips_b4",             200,  60,  4, _st(strip=1),                                 ["hadi_pass_a_strip<4,EU>"], [], {}),
    ("strips_b8",             300,  80,  4, _st(strip=1),                                 ["hadi_pass_a_strip<8,EU>"], [], {}),
    ("pairs",                 200,  60,  4, _st(strip=1, pair_strips=1),                  ["hadi_pass_a_pairs<EU>"], [], {}),
    ("paired_strips_rs_tab",  600,  40,  4, _st(strip=1),                                 ["hadi_pass_a_strip<8,EU,double,2>", "paired strips"], [], {}),
    ("pass_b1",               50,   300, 4, _st(),                                        ["hadi_pass_b1<16,EU>"], [], {}),
    ("pass_b2",               300,  264, 4, _st(col_prefetch=1, tile_interleave=1),       ["hadi_pass_b2<16,EU>"], [], {}),
    ("pass_b_seq",            40,   600, 4, _st(),                                        ["hadi_pass_b_seq<EU>"], [], {}),
    ("pass_a_seq",            1100, 20,  4, _st(),                                        ["hadi_pass_a_seq<EU>"], [], {}),
]


@pytest.mark.parametrize("name,m1,m2,n,tuning,want,absent,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_douglas_family(solver, name, m1, m2, n, tuning, want, absent, kw):
    _run_case(solver, name, tuning, want, m1, m2, 3, n, absent=absent, **kw)


@pytest.mark.parametrize("m1,m2,N,n,variant,kernel", [(300, 140, 3, 3, H.EU, "hadi_team_kernel<8>"), (256, 128, 10, 8, H.DIV, "hadi_team_kernel<4>")],
                         ids=["300x140", "256x128_dividends"])
def test_team_kernel(solver, m1, m2, N, n, variant, kernel):
    """The instance-resident launch stages RT (the reduced systems of the column chunks) per instance; with dividends the jump
    runs inside the launch (N = 10: all four dividend dates land on a step)."""
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the instance-resident launch needs the 256-CU device")
    strikes, grids, U0, _ = _batch(m1, m2, n)
    U = U0.copy()
    solver.set_tuning("team_launch", 1)
    try:
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, grids, U, variant=variant,
                               dividends=H.Dividends(*Cm.DIVS) if variant == H.DIV else None)
        d, state = solver.describe_last_sweep(), solver.get_tuning("team_launch")
    finally:
        solver.set_tuning("team_launch", -1)
    _has(d, [kernel])
    assert state == 1, (d, state)  # it ran, and the team protocol did not fail
    Uo, _ = _reference(m1, m2, N, n, variant=variant)
    _check("team %dx%d" % (m1, m2), U, None, Uo, None)


def _resident_pair(sv, m1, m2, N, n):
    """The mixed batch with "resident_sweep" = 1 and again with 0: (U, description, field of the streaming run)."""
    U, _, d = _sweep(sv, {"resident_sweep": 1}, m1, m2, N, n)
    Us, _, ds = _sweep(sv, {"resident_sweep": 0}, m1, m2, N, n)
    _has(d, [RESIDENT])
    _has(ds, [], [RESIDENT])
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13 and np.isfinite(U).all()
    return U, d


def test_resident_sweep_256_instances(solver):
    """hadi_sweep_resident<8> stages a block's invariants ONCE -- its own instance's: 256 instances on 300x80, every one
    against the oracle, and the field against the same call on the streaming kernels."""
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("256 instances are one round of blocks on the 256-CU device only")
    m1, m2, N, n = 300, 80, 3, 256
    U, d = _resident_pair(solver, m1, m2, N, n)
    _has(d, ["both passes of every step in one launch: " + RESIDENT, "hadi_pass_a_strip<8,EU> (strips of 11 rows)"])
    Uo, _ = _reference(m1, m2, N, n)
    _check("resident 300x80 x 256", U, None, Uo, None)


def test_resident_sweep_two_rounds_and_a_remainder(solver):
    """512x256, 500 = 256 + 122 + 122: a resident round and a remainder cut in two streaming halves -- each sub-batch must
    take its tables from its own offset.  First and last instance of every sub-batch plus the fixed subset."""
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the sub-batch sizes are the 256-CU device's")
    m1, m2, N, n = 512, 256, 3, 500
    try:
        U, d = _resident_pair(solver, m1, m2, N, n)
        _has(d, ["3 sub-batches of 256 122 122 instances", "for 1 sub-batches of one round: " + RESIDENT, "the others streaming"])
        rows = tuple(sorted({0, 255, 256, 377, 378, 499} | {0, 1, 7, 8, n - 2, n - 1}))
        Uo, _ = _reference(m1, m2, N, n, rows=rows)
        _check("resident 512x256 x 500, instances %s" % (rows,), U[list(rows)], None, Uo, None)
    finally:
        _batch.cache_clear()  # (half a gigabyte of payoffs: not kept for the rest of the session)


def test_two_streams(solver):
    """512x256 x 12 cut in two halves side by side: the second half's tables start at instance 6.  Bit for bit against one
    stream, and against the oracle."""
    m1, m2, N, n = 512, 256, 3, 12
    U1, _, d1 = _sweep(solver, {"streams": 1}, m1, m2, N, n)
    U2, _, d2 = _sweep(solver, {"streams": 2}, m1, m2, N, n)
    _has(d1, [], ["two streams"])
    _has(d2, ["two streams"])
    assert np.array_equal(U1, U2)
    Uo, _ = _reference(m1, m2, N, n)
    _check("two streams 512x256 x 12", U2, None, Uo, None)


# ---- B. variants on the streaming kernels -------------------------------------------------------------------------------
VARIANTS = [
    ("am_p_ring",        128, 64,  3, _st(),                            ["hadi_pass_a<2,1,", "AM-P"], ["strip"], dict(variant=H.AM)),
    ("am_pair_ring",     128, 64,  3, _st(american_p=0),                ["hadi_pass_a<2,1,", ",AM>"], ["strip", "AM-P"], dict(variant=H.AM)),
    ("am_div_ring",      128, 64,  10, _st(),                            ["hadi_pass_a<2,1,", "AM"], ["strip"], dict(variant=H.AM_DIV)),
    ("am_p_strips",      300, 140, 3, _st(strip=1),                     ["hadi_pass_a_strip<8,AM-P>"], [], dict(variant=H.AM)),
    ("am_pair_strips",   300, 140, 3, _st(strip=1, american_p=0),       ["hadi_pass_a_strip<8,AM>"], ["AM-P"], dict(variant=H.AM)),
    ("am_div_strips",    300, 140, 10, _st(strip=1),                     ["hadi_pass_a_strip<8,AM"], [], dict(variant=H.AM_DIV)),
    ("div_strips",       300, 140, 10, _st(strip=1),                     ["hadi_pass_a_strip<8,EU>"], [], dict(variant=H.DIV)),
    ("put_eu",           256, 128, 3, _st(),                            ["hadi_pass_a<4,1,", ",EU>"], [], dict(put=True)),
    ("put_am",           256, 128, 3, _st(),                            ["hadi_pass_a<4,1,", "AM"], [], dict(variant=H.AM, put=True)),
    ("fp32_ring",        512, 256, 3, _st(),                            ["hadi_pass_a<8,1,", "float"], ["strip"], dict(fp32=True)),
    ("fp32_paired_strips", 600, 40, 3, _st(strip=1),                    ["hadi_pass_a_strip<8,EU,float,2>"], [], dict(fp32=True)),
]


@pytest.mark.parametrize("name,m1,m2,N,tuning,want,absent,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variant_on_streaming_kernels(solver, name, m1, m2, N, tuning, want, absent, kw):
    """American sweeps in the P representation and on the explicit (U, lambda_bar) pair, dividend jumps (N = 10: with fewer
    than five steps no dividend date meets the reference's dating rule and the sweep is a European one), put boundary data,
    the fp32 state -- four instances, four v-grids."""
    _run_case(solver, name, tuning, want, m1, m2, N, 4, absent=absent, **kw)


# ---- C. predictor-corrector schemes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,theta,name", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning", [("ring", 128, 64, _st()), ("strips", 300, 80, _st(strip=1)),
                                               ("small_sch_b1", 50, 25, {"small_sch": 1}), ("small_sch_b2", 100, 20, {"small_sch": 1})],
                         ids=["ring", "strips", "small_sch_50x25", "small_sch_100x20"])
def test_scheme(solver, path, m1, m2, tuning, scheme, theta, name):
    """CS / MCS / HV: predictor and corrector both read the instance's v-tables; against tests/scheme_ref.py (the oracle for
    CS) per instance."""
    if path == "ring":
        want, absent = ["hadi_pass_a", ",%s>" % name], ["strip", SMALL_SCH]
    elif path == "strips":
        want, absent = ["hadi_pass_a_strip%s<8,EU,double,1,%s>" % ("" if name == "CS" else "_sch", name)], [SMALL_SCH]
    else:
        want, absent = [SMALL_SCH + "%d,%s>" % (1 if m1 <= 64 else 2, name)], []
    _run_case(solver, "%s %s" % (name, path), tuning, want, m1, m2, 3, 4, absent=absent, r_f=0.007, scheme=scheme, theta=theta)


# ---- D. launchers with V_0_i ---------------------------------------------------------------------------------------------
def _launcher_inputs(m1, m2, n0):
    """n0 options on the grids of for_strikes (the launchers ignore vec_v: the device rebuilds every instance's v-grid for its
    own V_0_i), V_0_i cycling through the free-V_0 candidates that obey the 30x rule at V = 5, d = 0.01."""
    strikes = Cm.well_conditioned_strikes(m1, n0)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0_ALT, strikes)
    assert Cm.interval_ratios(grids.Delta_s).max() <= Cm.COND_MAX
    cand = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)]
    v0s = [cand[k % len(cand)] for k in range(n0)]
    return strikes, grids, grids.call_payoff(strikes), v0s


def _oracle_launchers(p, grids, U0, v0s, eps=1e-6):
    """O.base_prices and O.jacobian of every option with that option's V_0 (options of one V_0 in one call, 16 threads)."""
    n0 = len(v0s)
    prices, J, base = np.empty(n0), np.empty((n0, 5)), np.empty(n0)
    for v0 in sorted(set(v0s)):
        r = np.array([k for k in range(n0) if v0s[k] == v0])
        g = (grids.Vec_s[r], grids.Vec_v[r], grids.Delta_s[r], grids.Delta_v[r])
        prices[r] = O.base_prices(p, Cm.S_0, v0, *g, U0[r], U0[r], threads=16)[0]
        J[r], base[r] = O.jacobian(p, Cm.S_0, v0, *g, U0[r], eps=eps, threads=16)
    return prices, J, base


def _check_launchers(name, prices, J, base, want):
    wp, wJ, wb = want
    ep, eb, eJ = np.abs(prices - wp).max(), np.abs(base - wb).max(), np.abs(J - wJ).max()
    print("%s: prices %.3e, base %.3e, J %.3e; |v0 column| >= %.3e" % (name, ep, eb, eJ, np.abs(J[:, 4]).min()))
    assert ep < 1e-9 and eb < 1e-9, (name, ep, eb)
    assert eJ < 2e-4, (name, eJ)
    # a kernel that solved the V_0 + eps group on the V_0 grid returns exactly 0 in the v0 column
    assert (np.abs(J[:, 4]) > 1e-2).all(), (name, J[:, 4])


LAUNCHERS = [
    # id               m1   m2   n0  tuning                                   the Jacobian's sweep names
    ("small_seq",      50,  25,  3,  {"small_seq": 1},                        ["hadi_small_seq_kernel<1>"]),
    ("small_seq2",     50,  25,  3,  {"small_seq": 1, "small_pairs": 1},      ["hadi_small_seq2_kernel<1>"]),
    ("ring",           128, 64,  3,  _st(),                                   ["hadi_pass_a<2,1,"]),
    ("strips",         300, 80,  2,  _st(strip=1),                            ["hadi_pass_a_strip<8,EU>"]),
    ("paired_strips",  600, 40,  2,  _st(strip=1),                            ["hadi_pass_a_strip<8,EU,double,2>"]),
    ("team",           300, 140, 1,  {"team_launch": 1},                      ["hadi_team_kernel<8>"]),
    ("resident",       300, 80,  42, {"resident_sweep": 1},                   [RESIDENT]),
]


@pytest.mark.parametrize("name,m1,m2,n0,tuning,want", LAUNCHERS, ids=[c[0] for c in LAUNCHERS])
def test_launchers_with_per_instance_V0(solver, name, m1, m2, n0, tuning, want):
    """compute_base_prices and compute_jacobian with V_0_i: 6 n0 instances, every group of n0 on its own v-grids and the sixth
    rebuilt for V_0_i + eps -- on the small-grid kernels, the ring, strips, paired strips, the team kernel (a whole Jacobian of
    one option) and the resident sweep (252 instances)."""
    if name in ("team", "resident") and solver.device_info()["compute_units"] != 256:
        pytest.skip("needs the 256-CU device")
    N = 4
    strikes, grids, U0, v0s = _launcher_inputs(m1, m2, n0)
    total = (m1 + 1) * (m2 + 1)
    args = (Cm.T, Cm.R_D, R_F, *MODEL, m1, m2, total, N, Cm.THETA, Cm.T / N, n0, grids)
    ws = H.DOWorkspace(n0, total)
    ws.U[...] = U0
    per = {"V_0_i": v0s}
    with _tuned(solver, tuning):
        prices = solver.compute_base_prices(Cm.S_0, -1.0, *args, ws, per_instance=per)
        J, base = solver.compute_jacobian(Cm.S_0, -1.0, *args, U0, per_instance=per)
        d = solver.describe_last_sweep()
        state = solver.get_tuning("team_launch")
    _has(d, want)
    assert name != "team" or state == 1, state
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, O.EU)
    _check_launchers(name, prices, J, base, _oracle_launchers(p, grids, U0, v0s))


@pytest.mark.parametrize("variant", ["american", "dividends"])
def test_jacobian_variants_with_per_instance_V0(solver, variant):
    """compute_jacobian_american / _dividends on the 128x64 ring (N = 10: all four dividend dates land on a step)."""
    m1, m2, n0, N = 128, 64, 3, 10
    strikes, grids, U0, v0s = _launcher_inputs(m1, m2, n0)
    total = (m1 + 1) * (m2 + 1)
    args = (Cm.T, Cm.R_D, R_F, *MODEL, m1, m2, total, N, Cm.THETA, Cm.T / N, n0, grids)
    ws = H.DOWorkspace(n0, total)
    ws.U[...] = U0
    per = {"V_0_i": v0s}
    div = H.Dividends(*Cm.DIVS)
    with _tuned(solver, _st()):
        if variant == "american":
            prices = solver.compute_base_prices_american(Cm.S_0, -1.0, *args, U0, ws, per_instance=per)
            J, base = solver.compute_jacobian_american(Cm.S_0, -1.0, *args, U0, per_instance=per)
        else:
            prices = solver.compute_base_prices_dividends(Cm.S_0, -1.0, *args, ws, div, per_instance=per)
            J, base = solver.compute_jacobian_dividends(Cm.S_0, -1.0, *args, U0, div, per_instance=per)
        d = solver.describe_last_sweep()
    _has(d, ["hadi_pass_a<2,1,", "AM" if variant == "american" else ",EU>"], ["strip"])
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, O.AM if variant == "american" else O.DIV,
                      None if variant == "american" else Cm.DIVS)
    _check_launchers(variant, prices, J, base, _oracle_launchers(p, grids, U0, v0s))


def _restated_launchers(m1, m2, N, theta, r_f, grids, U0, v0s, which, eps=1e-6):
    """oracle.base_prices / oracle.jacobian restated on tests/scheme_ref.py for the schemes the oracle does not know: forward
    differences in kappa, eta, sigma, rho on the v-grid rebuilt for the option's V_0, the v0 column from the grid rebuilt for
    V_0 + eps and picked at that node (V = 5, d = 0.01 as everywhere in the launchers)."""
    n0 = len(v0s)
    J, base = np.empty((n0, 5)), np.empty(n0)
    rho, sigma, kappa, eta = MODEL
    for k in range(n0):
        isx = O.find_s_index(grids.Vec_s[k], Cm.S_0)

        def price(model, v0):
            vv, dv = O.rebuild_variance(m2, v0)
            p = O.make_params(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, *model, O.EU)
            U = S.solve_one(p, grids.Vec_s[k], vv, grids.Delta_s[k], dv, U0[k], which)
            return U[isx + O.find_v_index(vv, v0) * (m1 + 1)]

        v0 = v0s[k]
        base[k] = price(MODEL, v0)
        bumped = [(rho, sigma, kappa + eps, eta), (rho, sigma, kappa, eta + eps), (rho, sigma + eps, kappa, eta),
                  (rho + eps, sigma, kappa, eta)]
        J[k, :4] = [(price(mdl, v0) - base[k]) / eps for mdl in bumped]
        J[k, 4] = (price(MODEL, v0 + eps) - base[k]) / eps
    return base.copy(), J, base


def test_launchers_with_per_instance_V0_on_the_small_scheme_kernel(solver):
    """scheme = MCS with "small_sch" = 1 on 50x25: hadi_small_sch_kernel carries the 6 n0 instances."""
    m1, m2, n0, N = 50, 25, 3, 4
    strikes, grids, U0, v0s = _launcher_inputs(m1, m2, n0)
    total = (m1 + 1) * (m2 + 1)
    args = (Cm.T, Cm.R_D, R_F, *MODEL, m1, m2, total, N, TH_MCS, Cm.T / N, n0, grids)
    ws = H.DOWorkspace(n0, total)
    ws.U[...] = U0
    per = {"V_0_i": v0s}
    with _tuned(solver, {"small_sch": 1}):
        prices = solver.compute_base_prices(Cm.S_0, -1.0, *args, ws, per_instance=per, scheme=H.SCHEME_MCS)
        J, base = solver.compute_jacobian(Cm.S_0, -1.0, *args, U0, per_instance=per, scheme=H.SCHEME_MCS)
        d = solver.describe_last_sweep()
    _has(d, [SMALL_SCH + "1,MCS>"])
    _check_launchers("MCS small_sch", prices, J, base, _restated_launchers(m1, m2, N, TH_MCS, R_F, grids, U0, v0s, S.MCS))


def test_multi_maturity_jacobian(solver):
    """compute_jacobian_multi_maturity on 128x64, three maturities: every (N, delta_t) group with its V_0 + eps group, against
    Cm.OracleSolver."""
    m1, m2, strikes3 = 128, 64, Cm.well_conditioned_strikes(128, 3)
    pts, ks = [], []
    for mi, (T_m, N_m) in enumerate(((0.5, 2), (1.0, 4), (1.5, 3))):
        for si, K in enumerate(strikes3):
            pts.append(H.CalibrationPoint(float(K), T_m, N_m, T_m / N_m, mi * 3 + si))
            ks.append(K)
    n, V0 = len(pts), Cm.V_0_ALT
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, V0, ks)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(ks)
    args = (Cm.S_0, V0, Cm.R_D, R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), Cm.THETA, pts, n, grids, U0)
    with _tuned(solver, _st()):
        J, base = solver.compute_jacobian_multi_maturity(*args)
        d = solver.describe_last_sweep()
    _has(d, ["hadi_pass_a<2,1,"], ["strip"])
    Jo, bo = Cm.OracleSolver().compute_jacobian_multi_maturity(*args)
    _check_launchers("multi-maturity", base, J, base, (bo, Jo, bo))


# ---- E. one V_0, different grids ----------------------------------------------------------------------------------------
SAME_V0 = Cm.V_0_ALT
ONE_V0 = [("ring_128x64", 128, 64, _st(), ["hadi_pass_a<2,1,"]), ("strips_300x80", 300, 80, _st(strip=1), ["hadi_pass_a_strip<8,EU>"]),
          ("small_50x25", 50, 25, {}, ["hadi_small_"])]


@pytest.mark.parametrize("name,m1,m2,tuning,want", ONE_V0[:2], ids=[c[0] for c in ONE_V0[:2]])
def test_parallel_DO_solve_picks_each_instances_row(solver, name, m1, m2, tuning, want):
    """One scalar V_0 that is a node of every grid, on a different row in each (hadi_pick_kernel finds it per instance)."""
    n, N = 4, 3
    strikes, grids, U0, v0s = _batch(m1, m2, n, False, SAME_V0)
    rows = [O.find_v_index(grids.Vec_v[k], SAME_V0) for k in range(n)]
    assert set(v0s) == {SAME_V0} and len(set(rows)) >= 2, rows
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    with _tuned(solver, tuning):
        prices = solver.parallel_DO_solve(n, Cm.S_0, SAME_V0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, grids, ws)
        d = solver.describe_last_sweep()
    _has(d, want)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, O.EU)
    cand = Cm.mixed_vgrid_candidates(m2, SAME_V0)
    worst = 0.0
    for k in range(n):
        V, _, dd = cand[k % len(cand)]
        sl = slice(k, k + 1)
        ref = O.base_prices(p, Cm.S_0, SAME_V0, grids.Vec_s[sl], grids.Vec_v[sl], grids.Delta_s[sl], grids.Delta_v[sl], U0[sl],
                            V=V, d=dd)[0][0]
        worst = max(worst, abs(prices[k] - ref))
    print("%s: parallel_DO_solve, rows of V_0 %s, worst price error %.3e" % (name, rows, worst))
    assert worst < 1e-9


@pytest.mark.parametrize("name,m1,m2,tuning,want", ONE_V0, ids=[c[0] for c in ONE_V0])
def test_greeks_and_ladder_on_each_instances_row(solver, name, m1, m2, tuning, want):
    """compute_greeks with the ladder: the v-derivative weights and the row of V_0 are the instance's own.  Against
    tests/greeks_ref.py on the oracle field of each instance, at the propagated bound of test_gpu_greeks.py."""
    n, N = 4, 3
    strikes, grids, U0, _ = _batch(m1, m2, n, False, SAME_V0)
    with _tuned(solver, tuning):
        greeks, lad = solver.compute_greeks(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, grids, U0.copy(), Cm.S_0, SAME_V0,
                                            ladder=True)
        d = solver.describe_last_sweep()
    _has(d, want)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, O.EU)
    worst, rows = 0.0, []
    for k in range(n):
        g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
        b, U, lam = G.boundary_vector(p, *g, U0[k])
        j0, i0 = G.find_node(g[1], SAME_V0), G.find_node(g[0], Cm.S_0)
        assert i0 >= 0 and j0 >= 0
        rows.append(j0)
        ref = G.ladder(p, *g, U, lam, j0, b)
        bound = G.propagated_bound(p, g[0], g[1], j0, np.abs(U).max())
        r, where = G.worst_ratio(lad[k], ref, bound)
        assert r <= 1.0, "instance %d node %d column %s: got %.17g ref %.17g bound %.3e" % (
            k, where[0], G.NAMES[where[1]], lad[k][where], ref[where], bound[where])
        assert np.array_equal(greeks[k], lad[k, i0])
        worst = max(worst, r)
    print("%s: Greeks ladder, rows of V_0 %s, worst |diff| / bound %.3e" % (name, rows, worst))
    assert len(set(rows)) >= 2, rows
