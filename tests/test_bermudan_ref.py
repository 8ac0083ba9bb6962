"""The Bermudan reference stepper (tests/bermudan_ref.py) against the oracle, on the CPU.

Without exercise steps it is oracle.solve bit for bit (EU and DIV, call and put).  With them it moves the field by far more than
the 1e-10 bound the GPU and emulator tests hold it to: dates against none, a schedule shifted by one step, one date dropped.  The
discrete scheme is not monotone (Bermudan minus European reaches -4.3e-5 of max|U|, put, 100x50x40): no ordering is asserted
tighter than that.  Every-step exercise is compared with the oracle's American field (Ikonen-Toivanen); the distance is first
order in dt and is recorded in DESIGN.md, not asserted as a tolerance.
"""
import numpy as np
import pytest

import bermudan_ref as BR
from common import DIVS, ETA, KAPPA, R_D, R_F, RHO, SIGMA, T, THETA, oracle_grids, oracle_params, put_payoff
from oracle import oracle as O

SHAPES = [(50, 25, 20), (100, 50, 40)]
K = 100.0


def problem(m1, m2, put):
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [K])
    if put:
        U0 = put_payoff(vs, [K], m2)
    return vs[0], vv[0], ds[0], dv[0], U0[0]


def ref(m1, m2, N, g, ex, div, put, scheme=0):
    return BR.solve_one(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *g, ex, dividends=DIVS if div else None,
                        put_strike=K if put else None, scheme=scheme)


@pytest.mark.parametrize("m1,m2,N", SHAPES)
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_no_exercise_is_the_oracle_bit_for_bit(m1, m2, N, div, put):
    g = problem(m1, m2, put)
    p = oracle_params(m1, m2, N, "DIV" if div else "EU", option_type=O.PUT if put else O.CALL, strikes=K if put else None)
    Uo, _, _ = O.solve(p, *g)
    assert np.array_equal(ref(m1, m2, N, g, [], div, put), Uo)


def test_canonical_dividends_pay_on_steps_4_8_11_16():
    assert BR.dividend_steps(20, T / 20, DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}


def schedule(N):
    return [N // 4, N // 2, (3 * N) // 4, N]


@pytest.mark.parametrize("m1,m2,N", SHAPES)
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_every_class_of_mistake_moves_the_field(m1, m2, N, div, put):
    """Each reference a GPU or emulator case uses differs from its European, shifted-schedule and one-date-short twin by at
    least 1e-4 of max|U|: six orders above the 1e-10 bound."""
    g = problem(m1, m2, put)
    ex = schedule(N)
    U = ref(m1, m2, N, g, ex, div, put)
    scale = np.abs(U).max()
    twins = {"none": [], "shifted": [n - 1 for n in ex], "dropped": ex[:1] + ex[2:]}
    for name, other in twins.items():
        shift = np.abs(U - ref(m1, m2, N, g, other, div, put)).max() / scale
        print("%s %s %dx%dx%d %s: %.3e" % ("put" if put else "call", "DIV" if div else "EU", m1, m2, N, name, shift))
        assert shift >= 1e-4, (name, shift)
    # no ordering tighter than the scheme's own non-monotonicity
    assert (U - ref(m1, m2, N, g, [], div, put)).min() / scale >= -1e-4


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_exercise_on_a_dividend_step(put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16, so a schedule containing 8 exercises at the END
    of a dividend step.  Swapping the order (exercise first, then the jump, which is what 'exercise at the end of step 7' is)
    gives another field."""
    m1, m2, N = 50, 25, 20
    g = problem(m1, m2, put)
    U = ref(m1, m2, N, g, [8, 16], True, put)
    V = ref(m1, m2, N, g, [7, 15], True, put)
    assert np.abs(U - V).max() / np.abs(U).max() >= 1e-4


@pytest.mark.parametrize("m1,m2,N", SHAPES)
def test_every_step_exercise_against_the_american_field(m1, m2, N):
    """Measured, not a tolerance: the distance is first order in dt (DESIGN.md section 2 records the figures)."""
    g = problem(m1, m2, True)
    U = ref(m1, m2, N, g, list(range(1, N + 1)), False, True)
    p = oracle_params(m1, m2, N, "AM", option_type=O.PUT, strikes=K)
    Ua, _, _ = O.solve(p, *g, U_0=g[4])
    dist = np.abs(U - Ua).max() / np.abs(Ua).max()
    print("every-step Bermudan put vs American %dx%dx%d: %.3e of max|U|" % (m1, m2, N, dist))
    assert np.isfinite(dist) and (U >= g[4] - 1e-12).all()


@pytest.mark.parametrize("scheme", [BR.CS, BR.MCS, BR.HV])
def test_schemes_without_exercise_are_scheme_ref(scheme):
    import scheme_ref as SR
    m1, m2, N = 50, 25, 20
    g = problem(m1, m2, False)
    p = oracle_params(m1, m2, N, "EU")
    assert np.array_equal(ref(m1, m2, N, g, [], False, False, scheme), SR.solve_one(p, *g, scheme))
    U = ref(m1, m2, N, g, schedule(N), False, False, scheme)
    assert np.abs(U - ref(m1, m2, N, g, [], False, False, scheme)).max() / np.abs(U).max() >= 1e-4


# ---- per-instance models and the dividend schedules of the event-domain tests --------------------------------------------------
def test_per_instance_models_without_events_are_the_oracle_bit_for_bit():
    import regimes as R
    m1, m2, N, n = 50, 25, 6, 4
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [K] * n)
    models = R.rotating_models(n, 1)
    for put in (False, True):
        U = put_payoff(vs, [K] * n, m2) if put else U0
        got = BR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [], models=models,
                             put_strikes=[K] * n if put else None)
        for k in range(n):
            p = O.make_params(m1, m2, N, T / N, THETA, R_D, R_F, *models[k], O.EU, option_type=O.PUT if put else O.CALL, strikes=K if put else None)
            assert np.array_equal(got[k], O.solve(p, vs[k], vv[k], ds[k], dv[k], U[k])[0]), (put, k)
        same = BR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [], put_strikes=[K] * n if put else None)
        assert not np.array_equal(got[1], same[1])  # (the models are read)
        assert np.array_equal(same[0], BR.solve_batch(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U, [],
                                                      models=[(RHO, SIGMA, KAPPA, ETA)] * n, put_strikes=[K] * n if put else None)[0])


def paying_steps_seen(monkeypatch, stepper):
    """The steps at whose start `stepper` calls the jump, with the dividend it pays: every Douglas step makes five operator calls
    (three products, two line solves), so the count of calls before a jump names its step."""
    calls, seen = [0], []
    op, jump = O.operator, BR.dividend_jump

    def counting(*a, **kw):
        calls[0] += 1
        return op(*a, **kw)

    def recording(vs, U, amount, pct, *a):
        assert calls[0] % 5 == 0
        seen.append((calls[0] // 5 + 1, amount, pct))
        return jump(vs, U, amount, pct, *a)

    monkeypatch.setattr(O, "operator", counting)
    monkeypatch.setattr(BR, "dividend_jump", recording)
    stepper()
    return seen


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_dividends_are_paid_on_exactly_the_steps_paying_steps_names(monkeypatch, put):
    import dividend_schedules as D
    import event_cases as E
    m1, m2 = 50, 25
    g = problem(m1, m2, put)
    cases = E.schedules_near_dividends(20, T / 20, T)[:3] + E.schedules_near_dividends(10, T / 10, T)[-6:]
    assert len(cases) == 9
    for c in cases:
        paid = D.paying_steps(c.N, c.dt, c.dividends[0])
        assert paid and paid == E.check(c, g[0])[0]
        run = lambda ex: BR.solve_batch(m1, m2, c.N, c.dt, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *(x[None] for x in g), ex,
                                        dividends=c.dividends, put_strikes=[K] if put else None)[0]
        seen = paying_steps_seen(monkeypatch, lambda: run(c.events))
        monkeypatch.undo()
        assert seen == [(n, c.dividends[1][q], c.dividends[2][q]) for n, q in sorted(paid.items())], (c.name, seen, paid)
        # ... and without events the stepper is the oracle's dividend sweep on that schedule, bit for bit
        p = O.make_params(m1, m2, c.N, c.dt, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, O.DIV, c.dividends, option_type=O.PUT if put else O.CALL,
                          strikes=K if put else None)
        assert np.array_equal(run([]), O.solve(p, *g)[0]), c.name
