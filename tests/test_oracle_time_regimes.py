"""CPU-only: the footing of the time-regime tests (tests/time_regimes.py).  At every regime T0 .. T7 the fp64 oracle's field
sits on its binary128 twin to round-off, so the project's field bound (1e-10 max|U_ref|) keeps its margin over the reference's
own error; lambda_bar's distance from the twin is measured and printed per regime and shape, and TIMES holds the worst value per
regime, from which the GPU bound follows (time_regimes.lambda_bound).  Every regime moves the field by far more than any bound
from the canonical-time field (theta 0.8, dt = 1 / N, same N), the theta regimes move it from each other (T0, T1, T2 at
dt = 1 / N; T7 against T6 at dt = 1e-6 on the shapes of T7_SHAPES): a kernel that used 0.8 where it was given another theta
cannot pass."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import regimes as R
import time_regimes as TR

SHAPES = [(50, 25, 20), (300, 40, 4), (600, 30, 3)]
#            id          variant   put
VARIANTS = [("eu_call",   O.EU,     False), ("am_put", O.AM, True), ("amdiv_call", O.AM_DIV, False)]
FIELD_XP, LAMBDA_XP = 5e-12, 1e-9  # (lambda_bar where dt >= 1e-2: the bound of test_oracle_xp.py)
SENSITIVITY = 1e-6
CASES = [(s, v, t) for s in SHAPES for v in VARIANTS for t in TR.TIME_IDS if v[1] != O.AM_DIV or TR.has_dividends(t)]
IDS = ["%dx%dx%d-%s-%s" % (s + (v[0], t)) for s, v, t in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(m1, m2, put):
    K = Cm.well_conditioned_strikes(m1, 1)
    v0 = next(v for v in (Cm.V_0, Cm.V_0_ALT) if Cm.interval_ratios(O.rebuild_variance(m2, v)[1])[0] <= Cm.COND_MAX)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, K, V0=v0)
    Cm.assert_well_conditioned(ds, dv)
    if put:
        U0 = Cm.put_payoff(vs, K, m2)
    return K, vs[0], vv[0], ds[0], dv[0], U0[0]


def _params(m1, m2, variant, put, theta, dt, N, K):
    divs = TR.dividends_at(N, dt) if variant in (O.DIV, O.AM_DIV) else None
    return O.make_params(m1, m2, N, dt, theta, *R.MODEL_RATES, *R.CANONICAL_MODEL, variant, divs,
                         option_type=O.PUT if put else O.CALL, strikes=np.array(K) if put else None)


@functools.lru_cache(maxsize=None)
def _field(m1, m2, variant, put, theta, dt, N):
    K, *g = _inputs(m1, m2, put)
    U, lam, _ = O.solve(_params(m1, m2, variant, put, theta, dt, N, K), *g, g[-1])
    assert np.isfinite(U).all() and (lam is None or np.isfinite(lam).all())
    return U, lam


def _regime(tid, N_row, variant):
    return TR.regime(tid, N_row, dividends=variant in (O.DIV, O.AM_DIV))


@pytest.mark.parametrize("shape,var,tid", CASES, ids=IDS)
def test_oracle_sits_on_its_binary128_twin(shape, var, tid):
    """Field <= 5e-12 of max|U| at every regime.  lambda_bar: the bound of test_oracle_xp.py where dt >= 1e-2; in the small-dt
    regimes its round-off is the field's divided by dt -- measured, printed, and never above the regime's entry in TIMES."""
    (m1, m2, N_row), (vid, variant, put) = shape, var
    theta, dt, N = _regime(tid, N_row, variant)
    K, *g = _inputs(m1, m2, put)
    U, lam = _field(m1, m2, variant, put, theta, dt, N)
    Ux, lx = O.solve_xp(_params(m1, m2, variant, put, theta, dt, N, K), *g, g[-1])
    assert np.isfinite(Ux).all() and (lx is None or np.isfinite(lx).all())
    e = np.abs(U - Ux).max() / np.abs(Ux).max()
    el = 0.0 if lam is None else np.abs(lam - lx).max() / max(1.0, np.abs(lx).max())
    print("%s %s %dx%dx%d (theta %g, dt %g): field %.2e, lambda_bar %.2e (max|lambda| %.2e)" % (
        tid, vid, m1, m2, N, theta, dt, e, el, 0.0 if lx is None else np.abs(lx).max()))
    assert e <= FIELD_XP, e
    assert el <= TR.TIME[tid][3], (el, TR.TIME[tid][3])
    assert dt < 1e-2 or el <= LAMBDA_XP, el


def test_the_lambda_entries_of_the_table():
    """Where dt >= 1e-2 the entry is below the bound of test_oracle_xp.py and the GPU bound is the project's 1e-8; in the
    small-dt regimes it is 30x the entry."""
    for tid in TR.TIME_IDS:
        theta, dt, N = TR.regime(tid, 4)
        xp = TR.TIME[tid][3]
        assert dt < 1e-2 or xp <= LAMBDA_XP, tid
        assert TR.lambda_bound(tid) == max(1e-8, 30.0 * xp)
        assert (tid in TR.SMALL_DT) == (dt < 1e-2)
    assert TR.ROTATION_LAMBDA == TR.lambda_bound("T6") and min(t[0] for t in TR.ROTATION) == TR.TIME["T6"][1]


@pytest.mark.parametrize("shape,var,tid", CASES, ids=IDS)
def test_every_regime_moves_the_field(shape, var, tid):
    """>= 1e-6 of max|U| from the canonical-time field: theta 0.8, dt = 1 / N, the same N (and, with dividends, the same
    fractions of the horizon)."""
    (m1, m2, N_row), (vid, variant, put) = shape, var
    theta, dt, N = _regime(tid, N_row, variant)
    U, _ = _field(m1, m2, variant, put, theta, dt, N)
    Uc, _ = _field(m1, m2, variant, put, *TR.canonical(N))
    d = np.abs(U - Uc).max() / np.abs(Uc).max()
    print("%s %s %dx%dx%d: %.2e of max|U| from the canonical-time field" % (tid, vid, m1, m2, N, d))
    assert d >= SENSITIVITY, d


@pytest.mark.parametrize("a,b", [("T0", "T1"), ("T0", "T2"), ("T1", "T2")])
@pytest.mark.parametrize("vid,variant,put", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("m1,m2,N_row", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_theta_regimes_move_the_field_from_each_other(m1, m2, N_row, vid, variant, put, a, b):
    Ua, _ = _field(m1, m2, variant, put, *_regime(a, N_row, variant))
    Ub, _ = _field(m1, m2, variant, put, *_regime(b, N_row, variant))
    d = np.abs(Ua - Ub).max() / np.abs(Ub).max()
    print("%s vs %s %s %dx%dx%d: %.2e of max|U|" % (a, b, vid, m1, m2, N_row, d))
    assert d >= SENSITIVITY, d


@pytest.mark.parametrize("put", [False, True], ids=["eu_call", "am_put"])
@pytest.mark.parametrize("m1,m2", TR.T7_SHAPES, ids=["%dx%d" % s for s in TR.T7_SHAPES])
def test_t7_moves_the_field_from_t6(m1, m2, put):
    """T6 and T7 share dt = 1e-6 and differ in theta alone: on every shape a GPU or emulator case runs T7 on, the two fields
    are >= 1e-6 of max|U| apart (European call and American put data)."""
    variant = O.AM if put else O.EU
    U6, _ = _field(m1, m2, variant, put, *TR.regime("T6", 3))
    U7, _ = _field(m1, m2, variant, put, *TR.regime("T7", 3))
    d = np.abs(U7 - U6).max() / np.abs(U6).max()
    print("T7 vs T6 %dx%d %s: %.2e of max|U|" % (m1, m2, "am_put" if put else "eu_call", d))
    assert d >= SENSITIVITY, d


@pytest.mark.parametrize("m1,m2", TR.T7_DROPPED, ids=["%dx%d" % s for s in TR.T7_DROPPED])
def test_the_shapes_t7_was_taken_off_do_fail_the_condition(m1, m2):
    """The record of why: on these shapes theta 1e-9 and theta 0.8 give the same field to < 1e-6 of max|U| at dt = 1e-6."""
    U6, _ = _field(m1, m2, O.EU, False, *TR.regime("T6", 3))
    U7, _ = _field(m1, m2, O.EU, False, *TR.regime("T7", 3))
    d = np.abs(U7 - U6).max() / np.abs(U6).max()
    print("T7 vs T6 %dx%d eu_call: %.2e of max|U| (dropped)" % (m1, m2, d))
    assert d < SENSITIVITY, d


def test_dividend_cases_pay_a_dividend():
    """dividends_at asserts it; here also that N_DIV steps are what makes it so: on the fixed N of T4 .. T7 nothing is paid."""
    for tid in TR.TIME_IDS:
        if not TR.has_dividends(tid):
            continue
        theta, dt, N = TR.regime(tid, 10, dividends=True)
        assert N >= 5 and len(TR.dividends_at(N, dt)[0]) == len(Cm.DIVS[0])
        fixed = TR.TIME[tid][2]
        if fixed is not None:
            with pytest.raises(AssertionError):
                TR.dividends_at(fixed, dt)


def test_rotation_never_repeats_a_dt_between_neighbours():
    for n in (2, 3, 4, 5, 7, 8, 256):
        for c in range(4):
            t = TR.time_rotation(n, c)
            assert len(t) == n and all(t[k][0] != t[k + 1][0] for k in range(n - 1))
    assert {t for c in range(4) for t in TR.time_rotation(1, c)} == set(TR.ROTATION)
    assert (TR.TIME["T4"][1], TR.TIME["T4"][2]) in TR.ROTATION and (TR.TIME["T6"][1], TR.TIME["T6"][2]) in TR.ROTATION
