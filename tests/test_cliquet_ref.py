"""The strike-fixing reference stepper (tests/cliquet_ref.py) against the oracle and a closed form, on the CPU.

Without fixings it is oracle.solve bit for bit (EU and DIV, call and put).  With them, every class of mistake a kernel or the host
code could make moves the field by far more than the 1e-10 bound the GPU and emulator tests hold it to: the reference node off by
one, a schedule shifted by one step, the other mode, a dropped fixing, a dropped weight.  And the model is sound: with a nearly
deterministic variance (sigma = 0.01, rho = 0, V_0 = eta) a forward-start call is S_0 e^{-r_f t1} BS(1, 1, r_d, r_f, sqrt(V_0),
T - t1), and the stepper reproduces it with the error the same grid makes on the plain call of maturity T - t1.
"""
import math

import numpy as np
import pytest

import bermudan_ref as BR
import cliquet_ref as QR
import common as Cm
from common import DIVS, ETA, KAPPA, R_D, R_F, RHO, SIGMA, T, THETA, oracle_grids, oracle_params, put_payoff
from oracle import oracle as O

K = 100.0


def problem(m1, m2, put, strike=K, V0=None):
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [strike], V0=Cm.v0_for(m2) if V0 is None else V0)
    if put:
        U0 = put_payoff(vs, [strike], m2)
    return vs[0], vv[0], ds[0], dv[0], U0[0]


def ref(m1, m2, N, g, fix, div=False, put=False, strike=K, scheme=0, **kw):
    return QR.solve_one(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *g, fix, dividends=DIVS if div else None,
                        put_strike=strike if put else None, scheme=scheme, **kw)


@pytest.mark.parametrize("m1,m2,N", [(50, 25, 20), (100, 50, 40)])
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_no_fixing_is_the_oracle_bit_for_bit(m1, m2, N, div, put):
    g = problem(m1, m2, put, V0=Cm.V_0)
    p = oracle_params(m1, m2, N, "DIV" if div else "EU", option_type=O.PUT if put else O.CALL, strikes=K if put else None)
    Uo, _, _ = O.solve(p, *g)
    assert np.array_equal(ref(m1, m2, N, g, [], div, put, ref_spot=K, mode=QR.RETURN, weights=[]), Uo)


def test_the_event_reads_before_it_writes_and_keeps_the_bits():
    vs = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    U = np.arange(15.0) + 0.1
    F = U.reshape(3, 5)
    S = QR.fixing(U, vs, 2, QR.SHARES, 0.0, U, 4, 2).reshape(3, 5)
    assert np.array_equal(S[:, 2], F[:, 2]) and np.array_equal(S, np.outer(F[:, 2], vs / 2.0))
    R = QR.fixing(U, vs, 0, QR.RETURN, 0.0, U, 4, 2).reshape(3, 5)
    assert np.array_equal(R, np.repeat(F[:, :1], 5, axis=1))
    W = QR.fixing(U, vs, 4, QR.RETURN, 0.5, 2.0 * U, 4, 2).reshape(3, 5)
    assert np.array_equal(W, np.repeat(F[:, 4:], 5, axis=1) + F)
    assert QR.find_node(vs, 3.0 + 5e-11) == 3 and QR.find_node(vs, 3.0 + 2e-10) == -1


SHAPES = [(50, 25, 20), (100, 50, 40), (200, 100, 80)]


@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_every_class_of_mistake_moves_the_field(m1, m2, N):
    """One fixing at N / 2, SHARES, the reference node at the strike.  Each twin differs from the reference by at least 1e-4 of
    max|U_ref|: six orders above the 1e-10 bound."""
    g = problem(m1, m2, False, V0=Cm.V_0)
    i_ref = QR.find_node(g[0], K)
    assert 1 < i_ref < m1
    U = ref(m1, m2, N, g, [N // 2], ref_spot=K)
    scale = np.abs(U).max()
    assert scale > 0
    twins = {"i_ref + 1": dict(fix=[N // 2], i_ref=i_ref + 1), "i_ref - 1": dict(fix=[N // 2], i_ref=i_ref - 1),
             "shifted schedule": dict(fix=[N // 2 - 1], ref_spot=K), "the other mode": dict(fix=[N // 2], ref_spot=K, mode=QR.RETURN),
             "dropped fixing": dict(fix=[])}
    for name, kw in twins.items():
        V = ref(m1, m2, N, g, kw.pop("fix"), **kw)
        shift = np.abs(U - V).max() / scale
        print("%dx%dx%d %s: %.3e" % (m1, m2, N, name, shift))
        assert shift >= 1e-4, (name, shift)


def test_a_dropped_weight_moves_a_capped_cliquet():
    """Four periods, local returns floored at 0 and capped at 5 %, coupons paid at the fixing dates: RETURN mode, weights 1, put
    boundary data."""
    m1, m2, N = 50, 25, 20
    vs, vv, ds, dv, _ = problem(m1, m2, True, V0=Cm.V_0)
    pay = np.tile(np.minimum(np.maximum(vs / K - 1.0, 0.0), 0.05), m2 + 1)
    g = (vs, vv, ds, dv, pay)
    U = ref(m1, m2, N, g, [5, 10, 15], put=True, ref_spot=K, mode=QR.RETURN, weights=[1.0, 1.0, 1.0])
    V = ref(m1, m2, N, g, [5, 10, 15], put=True, ref_spot=K, mode=QR.RETURN, weights=[1.0, 0.0, 1.0])
    shift = np.abs(U - V).max() / np.abs(U).max()
    print("dropped weight: %.3e" % shift)
    assert shift >= 1e-4
    W = ref(m1, m2, N, g, [5, 10, 15], put=True, ref_spot=K, mode=QR.SHARES, weights=[1.0, 1.0, 1.0])
    assert np.abs(U - W).max() / np.abs(U).max() >= 1e-4


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_fixing_on_a_dividend_step(put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16, so a schedule containing 8 fixes at the END of a
    dividend step.  The other order (fixing first, then the jump: 'fixing at the end of step 7') gives another field."""
    m1, m2, N = 50, 25, 20
    assert BR.dividend_steps(N, T / N, DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}
    g = problem(m1, m2, put)
    U = ref(m1, m2, N, g, [8, 16], True, put, ref_spot=K, weights=[0.0, 1.0])
    V = ref(m1, m2, N, g, [7, 15], True, put, ref_spot=K, weights=[0.0, 1.0])
    assert np.abs(U - V).max() / np.abs(U).max() >= 1e-4


@pytest.mark.parametrize("scheme", [QR.CS, QR.MCS, QR.HV])
def test_schemes_without_fixings_are_scheme_ref(scheme):
    import scheme_ref as SR
    m1, m2, N = 50, 25, 20
    g = problem(m1, m2, False, V0=Cm.V_0)
    p = oracle_params(m1, m2, N, "EU")
    assert np.array_equal(ref(m1, m2, N, g, [], scheme=scheme, ref_spot=K), SR.solve_one(p, *g, scheme))
    U = ref(m1, m2, N, g, [N // 2], scheme=scheme, ref_spot=K)
    assert np.abs(U - ref(m1, m2, N, g, [], scheme=scheme)).max() / np.abs(U).max() >= 1e-4


# ---- the closed form ------------------------------------------------------------------------------------------------------------
def black_scholes_call(S, Kk, r_d, r_f, vol, tau):
    Phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))
    d1 = (math.log(S / Kk) + (r_d - r_f + 0.5 * vol * vol) * tau) / (vol * math.sqrt(tau))
    return S * math.exp(-r_f * tau) * Phi(d1) - Kk * math.exp(-r_d * tau) * Phi(d1 - vol * math.sqrt(tau))


@pytest.mark.parametrize("m1,m2,N", SHAPES[1:], ids=["%dx%dx%d" % s for s in SHAPES[1:]])
@pytest.mark.parametrize("r_f", [0.0, 0.02])
def test_forward_start_call_against_the_closed_form(m1, m2, N, r_f):
    """sigma = 0.01, rho = 0, V_0 = eta = 0.04: the variance barely moves, so the at-the-money forward-start call fixed at
    t1 = T / 2 is S_0 e^{-r_f t1} BS(1, 1, r_d, r_f, 0.2, T - t1).  The grid's own error on the plain (T - t1)-year call is 1.3e-2 to
    2.9e-2; the event adds 2.1e-4 to 2.2e-4 to it (measured with this reference), and the bound is about twice that: 5e-4."""
    sig, rho, v0 = 0.01, 0.0, 0.04
    S0, t1 = Cm.S_0, 0.5 * T
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [S0], V0=v0)
    g = (vs[0], vv[0], ds[0], dv[0], U0[0])
    dt = T / N
    fs = QR.solve_one(m1, m2, N, dt, THETA, R_D, r_f, rho, sig, KAPPA, v0, *g, [N // 2], ref_spot=S0, mode=QR.SHARES)
    van = QR.solve_one(m1, m2, N // 2, dt, THETA, R_D, r_f, rho, sig, KAPPA, v0, *g, [])
    p_fs, p_van = BR.pick(g[0], g[1], fs, S0, v0, m1), BR.pick(g[0], g[1], van, S0, v0, m1)
    closed = S0 * math.exp(-r_f * t1) * black_scholes_call(1.0, 1.0, R_D, r_f, math.sqrt(v0), T - t1)
    bs = black_scholes_call(S0, S0, R_D, r_f, math.sqrt(v0), T - t1)
    extra = (p_fs - closed) - math.exp(-r_f * t1) * (p_van - bs)
    print("%dx%dx%d r_f %.2f: forward-start %.5f closed form %.5f error %.3e; plain call's error %.3e; the event adds %.3e"
          % (m1, m2, N, r_f, p_fs, closed, p_fs - closed, p_van - bs, extra))
    assert abs(extra) <= 5e-4
