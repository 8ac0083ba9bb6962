"""The knock-out reference stepper (tests/barrier_ref.py) against the oracle, on the CPU.

Without monitoring steps it is oracle.solve bit for bit (EU and DIV, call and put).  With them, every class of mistake a kernel
or the host code could make moves the field by far more than the 1e-10 bound the GPU and emulator tests hold it to: another
instance's barrier, a schedule shifted by one step, a dropped date, an up-only barrier for the double barrier, a forgotten
rebate, `<` for `<=` with the barrier on a node.  No ordering against the vanilla field is asserted: the discrete scheme is not
monotone (knock-out minus vanilla reaches +1.04 on put cases).
"""
import numpy as np
import pytest

import barrier_ref as KR
import common as Cm
from common import DIVS, ETA, KAPPA, R_D, R_F, RHO, SIGMA, T, THETA, oracle_grids, oracle_params, put_payoff
from oracle import oracle as O

K = 100.0
LO, UP = 0.7, 1.3  # the barriers, as fractions of the strike


def problem(m1, m2, put, strike=K, V0=None):
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [strike], V0=Cm.v0_for(m2) if V0 is None else V0)
    if put:
        U0 = put_payoff(vs, [strike], m2)
    return vs[0], vv[0], ds[0], dv[0], U0[0]


def ref(m1, m2, N, g, mon, div=False, put=False, strike=K, scheme=0, **kw):
    return KR.solve_one(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *g, mon, dividends=DIVS if div else None,
                        put_strike=strike if put else None, scheme=scheme, **kw)


@pytest.mark.parametrize("m1,m2,N", [(50, 25, 20), (100, 50, 40)])
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_no_monitoring_is_the_oracle_bit_for_bit(m1, m2, N, div, put):
    g = problem(m1, m2, put, V0=Cm.V_0)
    p = oracle_params(m1, m2, N, "DIV" if div else "EU", option_type=O.PUT if put else O.CALL, strikes=K if put else None)
    Uo, _, _ = O.solve(p, *g)
    assert np.array_equal(ref(m1, m2, N, g, [], div, put, lower=LO * K, upper=UP * K, rebate=3.0), Uo)


def test_knock_is_every_v_row_and_touching_knocks_out():
    vs = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    assert KR.knocked_nodes(vs, 1.0, 3.0).tolist() == [True, True, False, True, True]
    assert KR.knocked_nodes(vs, 1.0, 3.0, strict=True).tolist() == [True, False, False, False, True]
    assert KR.knocked_nodes(vs, None, 3.5).tolist() == [False, False, False, False, True]
    U = KR.knock(np.arange(15.0), KR.knocked_nodes(vs, 1.0, None), -7.0, 4, 2).reshape(3, 5)
    assert (U[:, :2] == -7.0).all() and np.array_equal(U[:, 2:], np.arange(15.0).reshape(3, 5)[:, 2:])


# the shapes of the emulator and GPU cases, with a time loop as short as theirs
SHAPES = [(50, 25, 8), (100, 20, 8), (300, 80, 3), (600, 30, 2), (40, 60, 8)]


def schedule(N):
    return sorted({max(1, N // 4), max(1, N // 2), N})


@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_every_class_of_mistake_moves_the_field(m1, m2, N, put):
    """Each twin differs from the reference by at least 1e-4 of max|U_ref|: six orders above the 1e-10 bound."""
    strike = Cm.well_conditioned_strikes(m1, 1)[0]
    g = problem(m1, m2, put, strike)
    Cm.assert_well_conditioned(g[2], g[3])
    mon = schedule(N)
    lo, up = LO * strike, UP * strike
    U = ref(m1, m2, N, g, mon, put=put, strike=strike, lower=lo, upper=up)
    scale = np.abs(U).max()
    assert scale > 0
    twins = {"another instance's barrier": dict(mon=mon, lower=0.8 * strike, upper=1.2 * strike),
             "shifted schedule": dict(mon=[n - 1 for n in mon if n > 1], lower=lo, upper=up),
             "dropped date": dict(mon=mon[:-1], lower=lo, upper=up),
             "up-only barrier": dict(mon=mon, lower=None, upper=up),
             "a rebate": dict(mon=mon, lower=lo, upper=up, rebate=1.0)}
    for name, kw in twins.items():
        V = ref(m1, m2, N, g, kw.pop("mon"), put=put, strike=strike, **kw)
        shift = np.abs(U - V).max() / scale
        print("%s %dx%dx%d %s: %.3e" % ("put" if put else "call", m1, m2, N, name, shift))
        assert shift >= 1e-4, (name, shift)


@pytest.mark.parametrize("m1,m2,N", SHAPES[:2] + SHAPES[4:], ids=["%dx%dx%d" % s for s in SHAPES[:2] + SHAPES[4:]])
def test_barrier_on_a_node_strict_comparison_moves_the_field(m1, m2, N):
    strike = Cm.well_conditioned_strikes(m1, 1)[0]
    g = problem(m1, m2, True, strike)
    vs = g[0]
    i_lo, i_up = int(np.searchsorted(vs, LO * strike)), int(np.searchsorted(vs, UP * strike))
    lo, up = float(vs[i_lo]), float(vs[i_up])
    U = ref(m1, m2, N, g, schedule(N), put=True, strike=strike, lower=lo, upper=up, rebate=0.5)
    V = ref(m1, m2, N, g, schedule(N), put=True, strike=strike, lower=lo, upper=up, rebate=0.5, strict=True)
    Ur = U.reshape(m2 + 1, m1 + 1)
    assert (Ur[:, i_lo] == 0.5).all() and (Ur[:, i_up] == 0.5).all() and (Ur[:, i_lo + 1] != 0.5).all()
    assert np.abs(U - V).max() / np.abs(U).max() >= 1e-4


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_knock_out_on_a_dividend_step(put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16, so a schedule containing 8 knocks out at the END
    of a dividend step.  The other order (knock-out first, then the jump: 'monitoring at the end of step 7') gives another field."""
    import bermudan_ref as BR
    m1, m2, N = 50, 25, 20
    assert BR.dividend_steps(N, T / N, DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}
    g = problem(m1, m2, put)
    U = ref(m1, m2, N, g, [8, 16], True, put, lower=LO * K, upper=UP * K)
    V = ref(m1, m2, N, g, [7, 15], True, put, lower=LO * K, upper=UP * K)
    assert np.abs(U - V).max() / np.abs(U).max() >= 1e-4


@pytest.mark.parametrize("scheme", [KR.CS, KR.MCS, KR.HV])
def test_schemes_without_monitoring_are_scheme_ref(scheme):
    import scheme_ref as SR
    m1, m2, N = 50, 25, 20
    g = problem(m1, m2, False, V0=Cm.V_0)
    p = oracle_params(m1, m2, N, "EU")
    assert np.array_equal(ref(m1, m2, N, g, [], scheme=scheme, lower=LO * K, upper=UP * K), SR.solve_one(p, *g, scheme))
    U = ref(m1, m2, N, g, schedule(N), scheme=scheme, lower=LO * K, upper=UP * K)
    assert np.abs(U - ref(m1, m2, N, g, [], scheme=scheme)).max() / np.abs(U).max() >= 1e-4


# ---- per-instance models and the dividend schedules of the event-domain tests --------------------------------------------------
def test_per_instance_models_without_events_are_the_oracle_bit_for_bit():
    import regimes as R
    m1, m2, N, n = 50, 25, 6, 4
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [K] * n)
    models = R.rotating_models(n, 1)
    for put in (False, True):
        U = put_payoff(vs, [K] * n, m2) if put else U0
        kw = dict(lower=LO * K, upper=UP * K, rebate=3.0, put_strikes=[K] * n if put else None)
        got = KR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [], models=models, **kw)
        for k in range(n):
            p = O.make_params(m1, m2, N, T / N, THETA, R_D, R_F, *models[k], O.EU, option_type=O.PUT if put else O.CALL, strikes=K if put else None)
            assert np.array_equal(got[k], O.solve(p, vs[k], vv[k], ds[k], dv[k], U[k])[0]), (put, k)
        same = KR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [], **kw)
        assert not np.array_equal(got[1], same[1])  # (the models are read)
        assert np.array_equal(same[0], KR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [],
                                                      models=[(RHO, SIGMA, KAPPA, ETA)] * n, **kw)[0])


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_dividends_are_paid_on_exactly_the_steps_paying_steps_names(monkeypatch, put):
    import dividend_schedules as D
    import event_cases as E
    from test_bermudan_ref import paying_steps_seen
    m1, m2 = 50, 25
    g = problem(m1, m2, put)
    cases = E.schedules_near_dividends(20, T / 20, T)[:3] + E.schedules_near_dividends(10, T / 10, T)[-6:]
    assert len(cases) == 9
    for c in cases:
        paid = D.paying_steps(c.N, c.dt, c.dividends[0])
        assert paid and paid == E.check(c, g[0])[0]
        lo, up = (E.floor_barrier(g[0][None])[0][0], None) if c.barrier == "floor" else (LO * K, UP * K)
        run = lambda mon: KR.solve_batch(m1, m2, c.N, c.dt, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *(x[None] for x in g), mon, lower=lo,
                                         upper=up, rebate=2.0, dividends=c.dividends, put_strikes=[K] if put else None)[0]
        seen = paying_steps_seen(monkeypatch, lambda: run(c.events))
        monkeypatch.undo()
        assert seen == [(n, c.dividends[1][q], c.dividends[2][q]) for n, q in sorted(paid.items())], (c.name, seen, paid)
        # ... and without monitoring the stepper is the oracle's dividend sweep on that schedule, bit for bit
        p = O.make_params(m1, m2, c.N, c.dt, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, O.DIV, c.dividends, option_type=O.PUT if put else O.CALL,
                          strikes=K if put else None)
        assert np.array_equal(run([]), O.solve(p, *g)[0]), c.name
