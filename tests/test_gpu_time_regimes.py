"""Every kernel family, variant, scheme and launcher at the theta and time-step regimes T0 .. T7 of tests/time_regimes.py, and
on batches whose instances carry different (delta_t_i, N_i).

The rest of the GPU suite runs theta = 0.8 with dt = 1 / N almost throughout.  Theta and dt select code paths and conditioning:
thdt = theta dt, RC_VTH = thdt v, a2i = I - theta dt A2, the strips' A0 weights divided by -theta dt (r_d - r_f) and their
explicit A1 share carried by (1 - theta) / theta (hadi_core.h, hadi_strip_step); at theta == 0 the host keeps the strips, the
team kernel and the resident sweep off (hadi_route.h) and at any theta > 0, however small, on; theta dt = 4 and 50 put the
un-pivoted pentadiagonal LU, the SPIKE reduced system and the Newton-refined reciprocal far from the identity; dt = 1e-6 makes
lambda_bar = (U_0 - P) / dt carry 1e6 times the field's round-off.  What the emulator cannot show is the gfx950 build.

No new launch configuration: rows, tuning keys and kernel names are those of test_gpu_mixed_vgrids.py (FAMILIES, VARIANTS,
SCHEMES) and test_gpu_regimes.py (TEAM, RES, SCHEME_PATHS, LAUNCH_SHAPES).  Canonical model at (r_d, r_f) = (0.025, 0.01).
Bounds: field 1e-10 max|U_ref| per instance on well-conditioned grids (asserted), fp32 state 2e-7 N, lambda_bar
time_regimes.lambda_bound (the project's 1e-8 max(1, max|lambda|) where dt >= 1e-2, 30x the oracle's own distance from its
binary128 twin in the small-dt regimes), prices 1e-9, J 2e-4, Greeks at the propagated bound of tests/greeks_ref.py.  Every case
asserts from describe_last_sweep() which kernel ran, that its reference is finite and that the regime moved the reference by
>= 1e-6 of max|U| from the canonical-time one (theta 0.8 -- the scheme's own theta for CS / MCS / HV -- dt = 1 / N, the same
N), and prints its observed maximum.  Exclusions (time_regimes.runs): dividend rows at T3, the fp32 state at the tiny-dt
regimes, T7 on the coarse s-grids where it does not move the field from T6."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm
import greeks_ref as G
import regimes as R
import scheme_ref as S
import time_regimes as TR
from test_gpu_mixed_vgrids import FAMILIES, OV, RESIDENT, SCHEMES, SMALL_SCH, VARIANTS, _field_errors, _has, _st, _tuned
from test_gpu_regimes import LAUNCH_SHAPES, RES, SCHEME_PATHS, SUBSET, TEAM, _inputs, _need_256, _off_strips

pytestmark = pytest.mark.gpu

RATES, M0 = R.MODEL_RATES, R.CANONICAL_MODEL
DIVIDEND = (H.DIV, H.AM_DIV)
TEAM_IDS = [t for t in TR.TIME_IDS if t not in TR.EXPLICIT]


def _divs(variant, N, dt):
    """The regime's dividend schedule as a hashable triple (None for the other variants); at least one date is paid (asserted)."""
    return tuple(tuple(x) for x in TR.dividends_at(N, dt)) if variant in DIVIDEND else None


def _sweep(sv, tuning, m1, m2, n, theta, times, variant=H.EU, put=False, scheme=0, fp32=False, divs=None):
    """One DO_timestepping under `tuning` -> (U_T, lambda_bar_T or None, description).  times: [(dt, N)] per instance; a batch
    of ONE (dt, N) goes through the scalars (delta_t_i = N_i = NULL), a batch of several through the per-instance arrays."""
    strikes, grids, U0, _ = _inputs(m1, m2, n, put)
    american = variant in (H.AM, H.AM_DIV)
    U, lam = U0.copy(), (np.zeros_like(U0) if american else None)
    per = None if len(set(times)) == 1 else TR.per_instance(times)
    with _tuned(sv, tuning):
        sv.DO_timestepping(m1, m2, max(t[1] for t in times), times[0][0], theta, *RATES, *M0, grids, U, variant=variant,
                           U_0=U0.copy() if american else None, lambda_bar=lam, dividends=H.Dividends(*divs) if divs else None,
                           per_instance=per, scheme=scheme, state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64,
                           option_type=H.PUT if put else H.CALL, strikes=list(strikes) if put else None)
        d = sv.describe_last_sweep()
        state = sv.get_tuning("team_launch")
    assert tuning.get("team_launch") != 1 or state == 1, (d, state)  # (the team protocol did not fail)
    return U, lam, d


@functools.lru_cache(maxsize=16)
def _reference(m1, m2, n, theta, times, variant=H.EU, put=False, scheme=0, fp32=False, divs=None, rows=None):
    """Every instance (or `rows`) with ITS (dt, N): the oracle on 16 threads (Douglas, Craig-Sneyd), tests/scheme_ref.py (MCS,
    HV).  Finite, asserted.  Computed once per case and left unchanged."""
    strikes, g, U0, _ = _inputs(m1, m2, n, put)
    r = list(range(n)) if rows is None else list(rows)
    ov = OV[variant]
    ks = np.asarray(strikes, dtype=np.float64)

    def params(dt, N, idx):
        return O.make_params(m1, m2, N, dt, theta, *RATES, *M0, ov, divs, scheme=1 if scheme == H.SCHEME_CRAIG_SNEYD else 0,
                             state_fp32=1 if fp32 else 0, option_type=O.PUT if put else O.CALL, strikes=ks[idx] if put else None)

    O.lib()
    if len(set(times)) == 1 and scheme not in (H.SCHEME_MCS, H.SCHEME_HV):
        Uo, lo, _ = O.solve_batch(params(*times[0], r), g.Vec_s[r], g.Vec_v[r], g.Delta_s[r], g.Delta_v[r], U0[r], U0[r], threads=16,
                                  want_lambda=True)
    else:
        def one(i):
            a = (g.Vec_s[i], g.Vec_v[i], g.Delta_s[i], g.Delta_v[i], U0[i])
            if scheme in (H.SCHEME_MCS, H.SCHEME_HV):
                return S.solve_one(params(*times[i], [i]), *a, S.MCS if scheme == H.SCHEME_MCS else S.HV), None
            return O.solve(params(*times[i], [i]), *a, U0[i])[:2]
        with ThreadPoolExecutor(16) as ex:
            out = list(ex.map(one, r))
        Uo = np.stack([o[0] for o in out])
        lo = None if out[0][1] is None else np.stack([o[1] for o in out])
    assert np.isfinite(Uo).all() and (lo is None or np.isfinite(lo).all())
    Uo.setflags(write=False)
    return Uo, lo


def _assert_moved(Uo, m1, m2, n, theta, times, variant=H.EU, scheme=0, rows=None, **kw):
    """The condition under the whole file: every instance's reference differs from the canonical-time one (theta 0.8 -- the
    scheme's theta for a predictor-corrector scheme -- dt = 1 / N, ITS N, dividends at the same fractions of the horizon) by
    >= 1e-6 of max|U|; instances ON the canonical time exempt -- a kernel that read the wrong theta or dt cannot pass."""
    ctheta = theta if scheme else TR.CANONICAL_THETA
    ctimes = tuple((Cm.T / N, N) for _, N in times)
    kw = dict(kw, divs=_divs(variant, times[0][1], Cm.T / times[0][1]))
    Uc, _ = _reference(m1, m2, n, ctheta, ctimes, variant=variant, scheme=scheme, rows=rows, **kw)
    moved = np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)
    idx = range(n) if rows is None else rows
    need = [j for j, i in enumerate(idx) if (theta, times[i]) != (ctheta, ctimes[i])]
    assert need and moved[need].min() >= 1e-6, moved


def _check(name, U, lam, Uo, lo, bound, lam_bound):
    e = _field_errors(U, Uo)
    msg = "%s: field error %.3e of max|U_ref| (instance %d of %d)" % (name, e.max(), int(e.argmax()), len(e))
    if lam is not None:
        el = np.abs(lam - lo).max() / max(1.0, np.abs(lo).max())
        msg += ", lambda_bar %.3e (bound %.1e, max|lambda| %.2e)" % (el, lam_bound, np.abs(lo).max())
    print(msg)
    assert e.max() <= bound, msg
    assert lam is None or (el <= lam_bound and np.abs(lo).max() > 0), msg


def _run(sv, name, tuning, want, absent, m1, m2, n, theta, times, lam_bound, rows=None, **kw):
    times = tuple(times)
    U, lam, d = _sweep(sv, tuning, m1, m2, n, theta, times, **kw)
    _has(d, want, absent)
    Uo, lo = _reference(m1, m2, n, theta, times, rows=rows, **kw)
    _assert_moved(Uo, m1, m2, n, theta, times, rows=rows, **kw)
    sel = slice(None) if rows is None else list(rows)
    N = max(t[1] for t in times)
    _check(name, U[sel], None if lam is None else lam[sel], Uo, lo, 2e-7 * N if kw.get("fp32") else 1e-10, lam_bound)
    return U, Uo


def _at(sv, name, tid, tuning, want, absent, m1, m2, n, N_row, rows=None, **kw):
    """One row at regime `tid`: the regime's theta, dt and N (dividend rows: its schedule), the row's kernel names -- at
    theta == 0 the shared-ring kernel of its class and no "strip" (_off_strips), at every other regime, T7 included, its own."""
    variant = kw.get("variant", H.EU)
    theta, dt, N = TR.regime(tid, N_row, dividends=variant in DIVIDEND)
    if tid in TR.EXPLICIT:
        want, absent = _off_strips(want, absent)
    return _run(sv, "%s %s" % (name, tid), tuning, want, absent, m1, m2, n, theta, [(dt, N)] * n, TR.lambda_bound(tid), rows=rows,
                divs=_divs(variant, N, dt), **kw)


# ---- a. Douglas families x T0 .. T7 --------------------------------------------------------------------------------------
FAMILY_RUNS = [(f, t) for f in FAMILIES for t in TR.TIME_IDS if TR.runs(t, f[1], f[2])]


@pytest.mark.parametrize("fam,tid", FAMILY_RUNS, ids=["%s-%s" % (f[0], t) for f, t in FAMILY_RUNS])
def test_family_at_time_regime(solver, fam, tid):
    name, m1, m2, n, tuning, want, absent, kw = fam
    _at(solver, name, tid, tuning, want, absent, m1, m2, n, 3, **kw)


# ---- b. variants x T0 .. T7 ----------------------------------------------------------------------------------------------
VARIANT_RUNS = [(v, t) for v in VARIANTS for t in TR.TIME_IDS
                if TR.runs(t, v[1], v[2], dividends=v[7].get("variant") in DIVIDEND, fp32=v[7].get("fp32", False))]


@pytest.mark.parametrize("var,tid", VARIANT_RUNS, ids=["%s-%s" % (v[0], t) for v, t in VARIANT_RUNS])
def test_variant_at_time_regime(solver, var, tid):
    """American P and the explicit pair, dividends (the canonical schedule at the same fractions of the regime's horizon; at
    least one date paid, asserted), put EU / AM, the fp32 state on the ring and on paired strips (T0, T1, T2, T4 only)."""
    name, m1, m2, N, tuning, want, absent, kw = var
    _at(solver, name, tid, tuning, want, absent, m1, m2, 4, N, **kw)


# ---- c. team kernel and resident sweep -----------------------------------------------------------------------------------
TEAM_RUNS = [(t, tid) for t in TEAM for tid in TEAM_IDS if TR.runs(tid, t[1], t[2], dividends=t[5] in DIVIDEND)]


@pytest.mark.parametrize("team,tid", TEAM_RUNS, ids=["%s-%s" % (t[0], tid) for t, tid in TEAM_RUNS])
def test_team_kernel_at_time_regime(solver, team, tid):
    _need_256(solver)
    name, m1, m2, N, n, variant, kernel = team
    _at(solver, name, tid, {"team_launch": 1}, [kernel], [], m1, m2, n, N, variant=variant)


def test_team_kernel_stays_off_at_theta_zero(solver):
    """hadi_team_grid: the team kernel's row step is the strips'.  "team_launch" = 1 and theta = 0: the streaming kernels
    answer, on the shared ring, and "team_launch" still reads 1."""
    _need_256(solver)
    name, m1, m2, N, n, variant, _ = TEAM[0]
    theta, dt, N = TR.regime("T3", N)
    _run(solver, "%s T3" % name, {"team_launch": 1}, ["hadi_pass_a<8,1,"], ["hadi_team_kernel", "strip"], m1, m2, n, theta, [(dt, N)] * n,
         TR.lambda_bound("T3"), variant=variant)


def _resident_pair(sv, name, theta, times, stays=True):
    """"resident_sweep" = 1 and again 0, as test_gpu_resident.py::test_inputs: the two fields to 1e-13, the resident one against
    the oracle (every instance) at 1e-10."""
    m1, m2, n = RES
    U, _ = _run(sv, name, {"resident_sweep": 1}, [RESIDENT, "hadi_pass_a_strip<8,EU> (strips of 11 rows)"] if stays else ["hadi_pass_a<8,1,"],
                [] if stays else [RESIDENT, "strip"], m1, m2, n, theta, times, 0.0)
    Us, _, ds = _sweep(sv, {"resident_sweep": 0}, m1, m2, n, theta, tuple(times))
    _has(ds, [], [RESIDENT])
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("  resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13 and np.isfinite(U).all()


@pytest.mark.parametrize("tid", TR.TIME_IDS)
def test_resident_sweep_at_time_regime(solver, tid):
    """At T3 the resident sweep stays off (hadi_resident_grid) and the streaming answer, on the shared ring, is right."""
    _need_256(solver)
    theta, dt, N = TR.regime(tid, 4)
    _resident_pair(solver, "resident %s" % tid, theta, [(dt, N)] * RES[2], stays=tid not in TR.EXPLICIT)


# ---- d. per-instance times -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FAMILIES)), ids=[f[0] for f in FAMILIES])
def test_family_with_rotating_times(solver, k):
    """theta 0.8, instance j on ROTATION[(j + k) % 4] = (5.0, 3), (1e-6, 3), (1/4, 4), (1e-3, 2): neighbours never share a dt,
    every instance against the oracle run with ITS (dt, N)."""
    name, m1, m2, n, tuning, want, absent, kw = FAMILIES[k]
    _run(solver, "%s rotated times c=%d" % (name, k), tuning, want, absent, m1, m2, n, TR.CANONICAL_THETA, TR.time_rotation(n, k),
         TR.ROTATION_LAMBDA, **kw)


def test_team_kernel_with_rotating_times(solver):
    _need_256(solver)
    name, m1, m2, _, n, variant, kernel = TEAM[0]
    _run(solver, "%s rotated times" % name, {"team_launch": 1}, [kernel], [], m1, m2, n, TR.CANONICAL_THETA, TR.time_rotation(n, 1),
         TR.ROTATION_LAMBDA, variant=variant)


def test_resident_sweep_with_rotating_times(solver):
    _need_256(solver)
    _resident_pair(solver, "resident rotated times", TR.CANONICAL_THETA, TR.time_rotation(RES[2], 2))


def test_rotating_times_on_the_graph_path():
    """A small batch with "graph" = 1 on a fresh handle: the first call captures the time loop (its per-step launches carry the
    longest N; every instance stops at its own), the second replays it; both against the oracle."""
    m1, m2, n = 128, 64, 4
    times = tuple(TR.time_rotation(n, 3))
    sv = H.HestonADI(0)
    try:
        sv.set_tuning("graph", 1)
        for call in range(2):
            g0 = Cm.graph_counts(sv)
            U, _, d = _sweep(sv, _st(), m1, m2, n, TR.CANONICAL_THETA, times)
            dg = Cm.graph_delta(g0, Cm.graph_counts(sv))
            _has(d, ["hadi_pass_a<2,1,"], ["strip"])
            assert (dg["captures"], dg["replays"], dg["drops"]) == ((1, 0, 0) if call == 0 else (0, 1, 0)), (call, dg)
            Uo, _ = _reference(m1, m2, n, TR.CANONICAL_THETA, times)
            _assert_moved(Uo, m1, m2, n, TR.CANONICAL_THETA, times)
            _check("graph path, call %d" % call, U, None, Uo, None, 1e-10, 0.0)
    finally:
        sv.close()


# ---- e. schemes ----------------------------------------------------------------------------------------------------------
SCHEME_TIMES = [("dt5", 5.0, 3), ("dt1e-6", 1e-6, 3)]
SCHEME_RUNS = [(p, s, t) for p in SCHEME_PATHS for s in SCHEMES for t in SCHEME_TIMES] + \
              [(p, SCHEMES[0], ("T3",) + TR.TIME["T3"][1:3]) for p in SCHEME_PATHS]


@pytest.mark.parametrize("path,sch,time", SCHEME_RUNS, ids=["%s-%s-%s" % (p[0], s[2], t[0]) for p, s, t in SCHEME_RUNS])
def test_scheme_at_time_regime(solver, path, sch, time):
    """CS / MCS / HV at their usual thetas against tests/scheme_ref.py (the oracle for CS) at dt = 5 and dt = 1e-6, and CS at
    T3 (theta = 0: forced strips fall back to the shared ring; MCS and HV divide by theta and are refused there)."""
    (pname, m1, m2, tuning), (scheme, theta, name), (tname, dt, N) = path, sch, time
    explicit = tname == "T3"
    theta = 0.0 if explicit else theta
    if pname == "ring":
        want, absent = ["hadi_pass_a", ",%s>" % name], ["strip", SMALL_SCH]
    elif pname == "strips" and explicit:
        want, absent = ["hadi_pass_a", "<8,1,", ",%s>" % name], ["strip", SMALL_SCH]
    elif pname == "strips":
        want, absent = ["hadi_pass_a_strip%s<8,EU,double,1,%s>" % ("" if name == "CS" else "_sch", name)], [SMALL_SCH]
    else:
        want, absent = [SMALL_SCH + "%d,%s>" % (1 if m1 <= 64 else 2, name)], []
    n = 4
    if explicit:  # (the canonical-time point of a scheme keeps the scheme's theta: here CS at its usual 0.5)
        times = ((dt, N),) * n
        U, _, d = _sweep(solver, tuning, m1, m2, n, theta, times, scheme=scheme)
        _has(d, want, absent)
        Uo, _ = _reference(m1, m2, n, theta, times, scheme=scheme)
        Uc, _ = _reference(m1, m2, n, SCHEMES[0][1], ((Cm.T / N, N),) * n, scheme=scheme)
        assert (np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)).min() >= 1e-6
        _check("CS %s T3" % pname, U, None, Uo, None, 1e-10, 0.0)
    else:
        _run(solver, "%s %s %s" % (name, pname, tname), tuning, want, absent, m1, m2, n, theta, [(dt, N)] * n, 0.0, scheme=scheme)


# ---- f. launchers and Greeks ---------------------------------------------------------------------------------------------
LAUNCH_TIMES = ("T1", "T4", "T6")


@pytest.mark.parametrize("tid", LAUNCH_TIMES)
@pytest.mark.parametrize("name,m1,m2,tuning,want_eu,want_amdiv", LAUNCH_SHAPES, ids=[s[0] for s in LAUNCH_SHAPES])
def test_launchers_at_time_regime(solver, name, m1, m2, tuning, want_eu, want_amdiv, tid):
    """compute_base_prices, compute_jacobian and parallel_DO_solve against Cm.OracleSolver: prices 1e-9, J 2e-4."""
    n0 = 3
    theta, dt, N = TR.regime(tid, 4)
    strikes, grids, U0, V0 = _inputs(m1, m2, n0)
    total = (m1 + 1) * (m2 + 1)
    args = (Cm.S_0, V0, N * dt, *RATES, *M0, m1, m2, total, N, theta, dt, n0, grids)
    ws, ws2 = H.DOWorkspace(n0, total), H.DOWorkspace(n0, total)
    ws.U[...] = U0
    ws2.U[...] = U0
    with _tuned(solver, tuning):
        prices = solver.compute_base_prices(*args, ws)
        dp = solver.describe_last_sweep()
        J, base = solver.compute_jacobian(*args, U0)
        dj = solver.describe_last_sweep()
        par = solver.parallel_DO_solve(n0, Cm.S_0, V0, m1, m2, N, N * dt, dt, theta, *RATES, *M0, grids, ws2)
        ds = solver.describe_last_sweep()
    for d in (dp, dj, ds):
        _has(d, want_eu)
    orc = Cm.OracleSolver()
    wso = H.DOWorkspace(n0, total)
    wso.U[...] = U0
    po = orc.compute_base_prices(*args, wso)
    Jo, bo = orc.compute_jacobian(*args, U0)
    canon = args[:12] + (N, TR.CANONICAL_THETA, Cm.T / N, n0, grids)
    pc = orc.compute_base_prices(*canon, wso)
    for x in (po, Jo, bo, pc):
        assert np.isfinite(x).all()
    moved = (np.abs(po - pc) / np.abs(pc)).min()
    assert moved >= 1e-6, moved  # (the regime moved every option's reference price from the canonical-time one)
    ep, eb, es, eJ = np.abs(prices - po).max(), np.abs(base - bo).max(), np.abs(par - po).max(), np.abs(J - Jo).max()
    print("%s %s: prices %.3e, base %.3e, parallel_DO_solve %.3e, J %.3e (max|J| %.3e)" % (name, tid, ep, eb, es, eJ, np.abs(Jo).max()))
    assert ep < 1e-9 and eb < 1e-9 and es < 1e-9, (ep, eb, es)
    assert eJ < 2e-4, eJ


GREEK_KINDS = [(H.EU, False), (H.AM, True)]


@pytest.mark.parametrize("tid", LAUNCH_TIMES)
@pytest.mark.parametrize("variant,put", GREEK_KINDS, ids=["EU_call", "AM_put"])
@pytest.mark.parametrize("name,m1,m2,tuning,want_eu,want_amdiv", LAUNCH_SHAPES, ids=[s[0] for s in LAUNCH_SHAPES])
def test_greeks_and_ladder_at_time_regime(solver, name, m1, m2, tuning, want_eu, want_amdiv, variant, put, tid):
    """compute_greeks with the spot ladder against tests/greeks_ref.py on the oracle's field, at the propagated bound of
    test_gpu_greeks.py.  The theta and lambda columns are where dt shows."""
    n = 2
    theta, dt, N = TR.regime(tid, 4)
    strikes, grids, U0, V0 = _inputs(m1, m2, n, put)
    with _tuned(solver, tuning):
        greeks, lad = solver.compute_greeks(m1, m2, N, dt, theta, *RATES, *M0, grids, U0.copy(), Cm.S_0, V0, variant=variant,
                                            option_type=H.PUT if put else H.CALL, strikes=list(strikes) if put else None, ladder=True)
        d = solver.describe_last_sweep()
    _has(d, want_eu if variant == H.EU else want_amdiv)
    worst = 0.0
    for k in range(n):
        def params(th, step):
            return O.make_params(m1, m2, N, step, th, *RATES, *M0, OV[variant], option_type=O.PUT if put else O.CALL,
                                 strikes=[strikes[k]] if put else None)
        g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
        u0 = U0[k] if variant == H.AM else None
        p = params(theta, dt)
        b, U, lam = G.boundary_vector(p, *g, U0[k], u0)
        assert np.isfinite(U).all()
        Uc = O.solve(params(TR.CANONICAL_THETA, Cm.T / N), *g, U0[k], u0)[0]
        assert np.abs(U - Uc).max() >= 1e-6 * np.abs(Uc).max()  # (the regime moved the reference)
        j0, i0 = G.find_node(g[1], V0), G.find_node(g[0], Cm.S_0)
        assert i0 >= 0 and j0 >= 0
        ref = G.ladder(p, *g, U, lam, j0, b)
        bound = G.propagated_bound(p, g[0], g[1], j0, np.abs(U).max())
        r, where = G.worst_ratio(lad[k], ref, bound)
        assert r <= 1.0, "instance %d node %d column %s: got %.17g ref %.17g bound %.3e" % (
            k, where[0], G.NAMES[where[1]], lad[k][where], ref[where], bound[where])
        assert np.array_equal(greeks[k], lad[k, i0])
        worst = max(worst, r)
    print("%s %s %s: Greeks ladder, worst |diff| / bound %.3e" % (name, tid, "AM put" if put else "EU call", worst))


def test_maturity_ladder_at_t4(solver):
    """One maturity_ladder call at theta dt = 4 (put data: call boundary data with r_f != 0 depend on N and are refused): every
    snapshot equals the call with N = that step bit for bit, and the oracle's price at 1e-9."""
    name, m1, m2, tuning, _, _ = LAUNCH_SHAPES[1]
    n = 3
    theta, dt, N = TR.regime("T4", 3)
    strikes, grids, U0, V0 = _inputs(m1, m2, n, True)
    kw = dict(option_type=H.PUT, strikes=list(strikes))
    with _tuned(solver, tuning):
        lad = solver.maturity_ladder(m1, m2, N, dt, theta, *RATES, *M0, grids, U0.copy(), Cm.S_0, V0, list(range(1, N + 1)), **kw)
        d = solver.describe_last_sweep()
        single = [solver.maturity_ladder(m1, m2, q, dt, theta, *RATES, *M0, grids, U0.copy(), Cm.S_0, V0, [q], **kw)[:, 0] for q in range(1, N + 1)]
    _has(d, ["hadi_pass_a<2,1,", "maturity ladder: %d snapshots" % N])
    worst = 0.0
    for q in range(1, N + 1):
        assert np.array_equal(lad[:, q - 1], single[q - 1]), q
        for k in range(n):
            p = O.make_params(m1, m2, q, dt, theta, *RATES, *M0, O.EU, option_type=O.PUT, strikes=[strikes[k]])
            Uo = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k])[0]
            assert np.isfinite(Uo).all()
            ref = Uo[O.find_s_index(grids.Vec_s[k], Cm.S_0) + O.find_v_index(grids.Vec_v[k], V0) * (m1 + 1)]
            worst = max(worst, abs(lad[k, q - 1] - ref))
    assert len({float(x) for x in lad[0]}) == N  # (the snapshots differ: the steps moved the price)
    print("maturity ladder T4: snapshots equal the per-N calls bit for bit; worst price error %.3e" % worst)
    assert worst < 1e-9


# ---- coverage ------------------------------------------------------------------------------------------------------------
def test_every_row_meets_every_time_regime():
    """The run lists against FAMILIES / VARIANTS / TEAM of the imported files: a row added there later meets every regime here
    but for the three exclusions of time_regimes.runs, or this fails."""
    assert TR.TIME_IDS == ["T%d" % k for k in range(8)]
    for f in FAMILIES:
        got = {t for ff, t in FAMILY_RUNS if ff[0] == f[0]}
        assert got == set(TR.TIME_IDS) - ({"T7"} if (f[1], f[2]) in TR.T7_DROPPED else set()), f[0]
        if "T7" in got:
            assert (f[1], f[2]) in TR.T7_SHAPES, f[0]
        if any("strip" in w or "pairs" in w for w in f[5]):
            assert "T7" in got and (f[1], f[2]) not in TR.T7_DROPPED or f[0] == "strips_b2", f[0]
            w, a = _off_strips(f[5], f[6])
            assert w != f[5] and "strip" in a and all("strip" not in x for x in w), f[0]
    for v in VARIANTS:
        got = {t for vv, t in VARIANT_RUNS if vv[0] == v[0]}
        want = set(TR.FP32_IDS) if v[7].get("fp32") else set(TR.TIME_IDS) - ({"T3"} if v[7].get("variant") in DIVIDEND else set())
        assert got == want and (v[7].get("fp32") or (v[1], v[2]) in TR.T7_SHAPES), v[0]
    assert {tid for t, tid in TEAM_RUNS if t[0] == TEAM[0][0]} == set(TEAM_IDS) == {tid for t, tid in TEAM_RUNS if t[0] == TEAM[1][0]}
    assert (RES[0], RES[1]) in TR.T7_SHAPES and all((t[1], t[2]) in TR.T7_SHAPES for t in TEAM)
    assert [s[2] for s in SCHEMES] == ["CS", "MCS", "HV"] and len(SCHEME_RUNS) == len(SCHEME_PATHS) * 7
    assert SUBSET[-1] < RES[2]
