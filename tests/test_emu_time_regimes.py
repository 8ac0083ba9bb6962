"""CPU-only: every kernel family of the wave emulator at the theta and time-step regimes T0 .. T7 of tests/time_regimes.py.
The rest of the emulator suite runs theta = 0.8 with dt = 1 / N; here theta is 0.5, 1, 2, 0 (the strips, the team kernel and the
resident sweep must be refused) and 1e-9 (the strips stay on, their A0 weights divided by theta dt q are ~7e16), theta dt is 4
and 50 (line systems far from the identity) and 8e-7 (the implicit stage is nearly the identity, lambda_bar carries 1 / dt).
Two instances per regime; one more batch per class rotates (delta_t_i, N_i) over four instances at theta 0.8
(time_regimes.time_rotation), each instance against the oracle run with ITS (dt, N).  Bounds: test_emu_kernel_logic._run (field
1e-11 max|U_ref|, lambda_bar 1e-9 max(1, max|lambda|)), 1e-10 for the resident sweep and the small scheme kernel as in their own
files; lambda_bar in the small-dt regimes at time_regimes.lambda_bound (30x the oracle's own distance from its binary128 twin,
which 1 / dt lifts above 1e-9 there: tests/test_oracle_time_regimes.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import regimes as R
import scheme_ref as S
import test_emu_small_sch as ES
import time_regimes as TR
from test_emu_kernel_logic import _P, _plan, emu  # noqa: F401  (emu: the module's fixture)
from test_emu_regimes import CLASSES, EMU_AMP, INDEX, TOL, _inputs, _tuning
from test_emu_resident import emu as emu_resident  # noqa: F401
from test_emu_small_sch import emu as emu_small_sch  # noqa: F401

_ip = C.POINTER(C.c_int)
RATES, MODEL = R.MODEL_RATES, R.CANONICAL_MODEL
DIVIDEND = (O.DIV, O.AM_DIV)
STRIP_CLASSES = [c[0] for c in CLASSES if c[8] is not None and c[8][2]]
TEAM_CLASSES = [c[0] for c in CLASSES if c[7].get("small") == 4]
REFUSED, UNSUPPORTED = 3, 3  # emu_solve: the team kernel's shape is not admitted / per-instance step grids with dividends


def _lambda_tol(tid):
    return TR.lambda_bound(tid) if tid in TR.SMALL_DT else 1e-9


def _emu(emu, m1, m2, variant, tw, theta, times, grids, small=0, scheme=0, put=False, divs=None, uniform=True):
    """emu_solve on `times` = [(dt, N)] per instance; uniform: all equal, passed through the scalars (N_i = dt_i = NULL)."""
    strikes, vs, vv, ds, dv, U0 = grids
    n = len(strikes)
    ks = np.array(strikes, dtype=np.float64)
    U, lam = U0.copy(), np.zeros_like(U0)
    par = np.ascontiguousarray(np.tile(np.array(MODEL, dtype=np.float64), (n, 1)))
    dd = [np.array(x, dtype=np.float64) for x in (divs or ([], [], []))]
    Ni, dti = np.array([t[1] for t in times], dtype=np.int32), np.array([t[0] for t in times], dtype=np.float64)
    assert not uniform or len(set(times)) == 1
    rc = emu.emu_solve(n, m1, m2, times[0][1], C.c_double(times[0][0]), C.c_double(theta), C.c_double(RATES[0]), C.c_double(RATES[1]),
                       _P(par), variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), tw, len(dd[0]), _P(dd[0]), _P(dd[1]),
                       _P(dd[2]), 64, small, scheme, _P(ks) if put else None, None if uniform else Ni.ctypes.data_as(_ip),
                       None if uniform else _P(dti))
    return rc, U, lam


def _oracle(m1, m2, variant, theta, dt, N, grids, k, put, divs=None):
    strikes, vs, vv, ds, dv, U0 = grids
    p = O.make_params(m1, m2, N, dt, theta, *RATES, *MODEL, variant, divs, option_type=O.PUT if put else O.CALL,
                      strikes=np.array(strikes[k:k + 1]) if put else None)
    Uo, lo, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k], U0[k])
    assert np.isfinite(Uo).all() and (lo is None or np.isfinite(lo).all())
    return Uo, lo


def _compare(name, U, lam, m1, m2, variant, theta, times, grids, put, tol, lam_tol, divs=None):
    worst = wl = 0.0
    for k, (dt, N) in enumerate(times):
        Uo, lo = _oracle(m1, m2, variant, theta, dt, N, grids, k, put, divs)
        worst = max(worst, np.abs(U[k] - Uo).max() / np.abs(Uo).max())
        if lo is not None:
            wl = max(wl, np.abs(lam[k] - lo).max() / max(1.0, np.abs(lo).max()))
    print("%s: field %.2e, lambda_bar %.2e" % (name, worst, wl))
    assert worst < tol and wl < lam_tol, (worst, wl)


def _route_desc(emu, m1, m2, n, variant, theta, tuning, amp):
    """hadi_describe_last_sweep's text for the class's call on the streaming kernels of the 256-CU device (emu_route)."""
    keys = dict(tuning, small_grid=0, team_launch=0, resident_sweep=0)
    arr = (C.c_int * 16)(256, n, m1, m2, variant, 0, 0, 0, 0, 0, 0, int(variant in DIVIDEND), 1, 0, int(amp), 0)
    o, subs, desc = (C.c_longlong * 15)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
    emu.emu_route.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    rc = emu.emu_route(arr, theta, ",".join("%s=%d" % kv for kv in keys.items()).encode(), o, subs, 64, desc, 1024)
    assert rc == 0, (rc, o[0])
    return desc.value.decode()


FAMILY_RUNS = [(c, tid) for c in CLASSES for tid in TR.TIME_IDS if c[5] not in DIVIDEND or TR.has_dividends(tid)]


@pytest.mark.parametrize("cls,tid", FAMILY_RUNS, ids=["%s-%s" % (c[0], t) for c, t in FAMILY_RUNS])
def test_family_at_time_regime(emu, cls, tid):
    name, tuning, m1, m2, N_row, variant, tw, kw, plan = cls
    theta, dt, N = TR.regime(tid, N_row, dividends=variant in DIVIDEND)
    n, put = 2, kw.get("put", False)
    grids = _inputs(m1, m2, n, put)
    divs = TR.dividends_at(N, dt) if variant in DIVIDEND else None
    with _tuning(emu, tuning):
        assert plan is None or _plan(emu, m1, m2, n, tw) == plan, (_plan(emu, m1, m2, n, tw), plan)
        rc, U, lam = _emu(emu, m1, m2, variant, tw, theta, [(dt, N)] * n, grids, divs=divs, **kw)
    if name in STRIP_CLASSES:  # hadi_no_strips: the route keeps the strips at every theta > 0, however small, and drops them at 0
        d = _route_desc(emu, m1, m2, n, variant, theta, tuning, kw.get("scheme") == EMU_AMP)
        assert ("strip" in d or "pairs" in d) == (tid not in TR.EXPLICIT), (tid, d)
        assert tid not in TR.EXPLICIT or "hadi_pass_a<%d,%d," % plan[:2] in d, d
    if name in TEAM_CLASSES and tid in TR.EXPLICIT:
        assert rc == REFUSED, rc  # the team kernel's row step is the strips': off at theta == 0 (hadi_team_grid)
        return
    assert rc == 0, rc
    _compare("%s %s" % (name, tid), U, lam, m1, m2, variant, theta, [(dt, N)] * n, grids, put, TOL, _lambda_tol(tid), divs)


@pytest.mark.parametrize("cls", CLASSES, ids=[c[0] for c in CLASSES])
def test_family_with_rotating_times(emu, cls):
    """Four instances at theta 0.8 on (5.0, 3), (1e-6, 3), (1/4, 4), (1e-3, 2), rotated by the class index: every kernel reads
    ITS instance's dt (ipar.dt, thdt and the tables built from them) and stops at ITS N.  emu_solve has no per-instance dividend
    tables: the dividend classes assert the refusal."""
    name, tuning, m1, m2, _, variant, tw, kw, plan = cls
    n, put = 4, kw.get("put", False)
    times = TR.time_rotation(n, INDEX[name])
    grids = _inputs(m1, m2, n, put)
    with _tuning(emu, tuning):
        rc, U, lam = _emu(emu, m1, m2, variant, tw, TR.CANONICAL_THETA, times, grids, divs=Cm.DIVS if variant in DIVIDEND else None,
                          uniform=False, **kw)
    if variant in DIVIDEND:
        assert rc == UNSUPPORTED, rc
        return
    assert rc == 0, rc
    _compare("%s rotated times c=%d" % (name, INDEX[name]), U, lam, m1, m2, variant, TR.CANONICAL_THETA, times, grids, put, TOL,
             TR.ROTATION_LAMBDA)


def test_the_rotated_batches_reach_every_kernel_class():
    """The team rows (small = 4) without dividends and every strip class admit per-instance times; only dividends refuse."""
    admitted = {c[0] for c in CLASSES if c[5] not in DIVIDEND}
    assert {"team", "team_put"} <= admitted and set(STRIP_CLASSES) - {"dividends_strips"} <= admitted
    assert set(TEAM_CLASSES) == {"team", "team_put", "team_div"}
    assert {"strips", "strips_forced_am", "strips_put_am", "pairs", "paired_strips", "american_p_strips"} <= set(STRIP_CLASSES)
    assert TR.TIME["T3"][0] == 0.0 and 0.0 < TR.TIME["T7"][0] < 1e-8


# ---- the resident sweep -------------------------------------------------------------------------------------------------
def _resident(emu_resident, m1, m2, theta, times, grids, put, uniform):
    strikes, vs, vv, ds, dv, U0 = grids
    n = len(strikes)
    par = np.ascontiguousarray(np.tile(np.array(MODEL, dtype=np.float64), (n, 1)))
    ks = np.ascontiguousarray(strikes, dtype=np.float64)
    Ni, dti = np.array([t[1] for t in times], dtype=np.int32), np.array([t[0] for t in times], dtype=np.float64)
    U, P = U0.copy(), C.c_int(0)
    rc = emu_resident.emu_solve_resident(n, m1, m2, times[0][1], C.c_double(times[0][0]), C.c_double(theta), C.c_double(RATES[0]),
                                         C.c_double(RATES[1]), _P(par), _P(vs), _P(vv), _P(ds), _P(dv), _P(U), 64,
                                         None if uniform else Ni.ctypes.data_as(_ip), None if uniform else _P(dti), C.byref(P), _P(ks),
                                         1 if put else 0)
    return rc, U


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
@pytest.mark.parametrize("tid", TR.TIME_IDS + ["rotated"])
def test_resident_sweep_at_time_regime(emu_resident, tid, put):
    m1, m2 = 300, 40
    if tid == "rotated":
        theta, times = TR.CANONICAL_THETA, TR.time_rotation(4, 1 + put)
    else:
        theta, dt, N = TR.regime(tid, 2)
        times = [(dt, N)] * 2
    grids = _inputs(m1, m2, len(times), put)
    rc, U = _resident(emu_resident, m1, m2, theta, times, grids, put, tid != "rotated")
    if tid in TR.EXPLICIT:
        assert rc == REFUSED  # no strips at theta == 0, and no resident sweep without strips (hadi_resident_grid)
        return
    assert rc == 0, rc
    _compare("resident %s %s" % (tid, "put" if put else "call"), U, None, m1, m2, O.EU, theta, times, grids, put, 1e-10, 1.0)


# ---- hadi_small_sch_kernel ----------------------------------------------------------------------------------------------
def _small_sch(emu_small_sch, m1, m2, scheme, theta, times):
    n = len(times)
    strikes, vs, vv, ds, dv, U0 = _inputs(m1, m2, n, False)
    par8 = np.array([list(MODEL) + [dt, N, 0.0, 0.0] for dt, N in times])
    U = np.ascontiguousarray(U0.copy())
    rc = emu_small_sch.emu_small_sch(n, m1, m2, C.c_double(theta), C.c_double(RATES[0]), C.c_double(RATES[1]), _P(par8), _P(vs), _P(vv),
                                     _P(ds), _P(dv), _P(U), scheme, 64, None)
    if rc:
        return rc, 0.0
    worst = 0.0
    for k, (dt, N) in enumerate(times):
        p = O.make_params(m1, m2, N, dt, theta, *RATES, *MODEL, O.EU)
        Uo = S.solve_one(p, vs[k], vv[k], ds[k], dv[k], U0[k], scheme)
        assert np.isfinite(Uo).all()
        worst = max(worst, np.abs(U[k] - Uo).max() / np.abs(Uo).max())
    return 0, worst


@pytest.mark.parametrize("tid", TR.TIME_IDS + ["rotated"])
@pytest.mark.parametrize("scheme,usual,name", ES.SCHEMES, ids=[s[2] for s in ES.SCHEMES])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_small_scheme_kernel_at_time_regime(emu_small_sch, m1, m2, scheme, usual, name, tid):
    """CS / MCS / HV at the regime's theta and dt; the rotated batch at the scheme's usual theta.  MCS and HV divide by theta:
    the library refuses them at theta == 0 and so does the driver; CS runs its explicit step."""
    if tid == "rotated":
        theta, times = usual, TR.time_rotation(4, scheme + (m1 > 64))
    else:
        theta, dt, N = TR.regime(tid, 2)
        times = [(dt, N)] * 2
    rc, worst = _small_sch(emu_small_sch, m1, m2, scheme, theta, times)
    if tid in TR.EXPLICIT and scheme != S.CS:
        assert rc == REFUSED, rc
        return
    assert rc == 0, rc
    print("small_sch %s %dx%d %s: field %.2e" % (name, m1, m2, tid, worst))
    assert worst <= 1e-10  # (the bound of test_emu_small_sch._check)
