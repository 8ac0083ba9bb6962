"""The Bates reference stepper (tests/jumps_ref.py) against the oracle and against the semi-analytic Bates price, on the CPU.

With lambda = 0 it is oracle.solve bit for bit (EU and DIV, call and put).  The generator annihilates constants and the function
s (jumps neither create nor destroy money; the forward is a martingale on the grid).  With jumps the split scheme converges to
the characteristic-function price at the rate plain Heston does, and each class of mistake in the generator moves the price by
far more than the bounds the GPU and emulator tests hold the fields to.
"""
import numpy as np
import pytest

import bermudan_ref as BR
import common as Cm
import jumps_ref as JR
from common import DIVS, ETA, KAPPA, R_D, R_F, RHO, SIGMA, T, THETA, oracle_grids, oracle_params, put_payoff
from oracle import oracle as O

K = 100.0
# (lambda, mu_J, sigma_J): the three parameter sets of the accuracy table
JUMP_SETS = [(0.5, -0.10, 0.15), (2.0, -0.05, 0.10), (0.3, 0.10, 0.30)]
IDS = ["lam%.1f_mu%+.2f_sig%.2f" % s for s in JUMP_SETS]


def problem(m1, m2, put=False, strike=K, V0=Cm.V_0):
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [strike], V0=V0)
    if put:
        U0 = put_payoff(vs, [strike], m2)
    return vs[0], vv[0], ds[0], dv[0], U0[0]


@pytest.mark.parametrize("m1,m2,N", [(50, 25, 20), (100, 50, 40)])
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_zero_intensity_is_the_oracle_bit_for_bit(m1, m2, N, div, put):
    g = problem(m1, m2, put)
    p = oracle_params(m1, m2, N, "DIV" if div else "EU", option_type=O.PUT if put else O.CALL, strikes=K if put else None)
    Uo, _, _ = O.solve(p, *g)
    U = JR.solve_one(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *g, lam=0.0, mu_j=-0.1, sigma_j=0.15,
                     dividends=DIVS if div else None, put_strike=K if put else None)
    assert np.array_equal(U, Uo)


@pytest.mark.parametrize("m1", [50, 100, 300, 600])
@pytest.mark.parametrize("lam,mu,sig", JUMP_SETS, ids=IDS)
def test_generator_annihilates_constants_and_the_spot(m1, lam, mu, sig):
    """G 1 = 0 and G s = 0 to 1e-12 of max|s| (measured: about 1e-14); row 0 is all zero."""
    vs = oracle_grids(m1, 8, [K])[0][0]
    G = JR.generator(vs, mu, sig)
    r1, rs = np.abs(G @ np.ones_like(vs)).max(), np.abs(G @ vs).max()
    print("m1 = %d (%g, %g): |G 1| = %.2e, |G s| = %.2e, max|s| = %g" % (m1, mu, sig, r1, rs, vs.max()))
    assert r1 <= 1e-12 * vs.max() and rs <= 1e-12 * vs.max()
    assert not G[0].any()


def test_generator_pieces():
    """J is a stochastic matrix up to the extrapolation (rows sum to 1, entries beyond the last interval may be negative), D is
    exact on linear functions."""
    vs = oracle_grids(100, 8, [K])[0][0]
    J = JR.expectation_matrix(vs, -0.1, 0.15)
    assert np.abs(J[1:].sum(axis=1) - 1.0).max() < 1e-13
    assert np.abs(J[1:] @ vs - vs[1:] * (1.0 + JR.kbar(-0.1, 0.15))).max() < 1e-12 * vs.max()
    D = JR.derivative_matrix(vs)
    assert np.abs(D[1:] @ vs - 1.0).max() < 1e-12 and np.abs(D @ np.ones_like(vs)).max() < 1e-12


def price(m1, m2, N, lam, mu, sig, **mut):
    g = problem(m1, m2)
    U = JR.solve_one(m1, m2, N, T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, *g, lam=lam, mu_j=mu, sigma_j=sig, **mut)
    return BR.pick(g[0], g[1], U, Cm.S_0, Cm.V_0, m1)


_PRICES = {}


def coarse(lam, mu, sig):
    """The 100x50x100 reference price, computed once per parameter set."""
    if (lam, mu, sig) not in _PRICES:
        _PRICES[(lam, mu, sig)] = price(100, 50, 100, lam, mu, sig)
    return _PRICES[(lam, mu, sig)]


def test_semi_analytic_price_without_jumps_is_hestons():
    p = JR.bates_call_semi_analytic(Cm.S_0, K, T, R_D, R_F, KAPPA, ETA, SIGMA, RHO, Cm.V_0, 0.0, -0.1, 0.15)
    assert abs(p - 8.8948693600540167) < 5e-11  # (the reference's convergence target: tests/test_reference_pins.py)


@pytest.mark.parametrize("lam,mu,sig", JUMP_SETS, ids=IDS)
def test_accuracy_against_the_semi_analytic_price(lam, mu, sig):
    """Within 1.1e-2 at 100x50x100 (plain Heston's own error on that grid); at least 3x smaller at 200x100x400."""
    exact = JR.bates_call_semi_analytic(Cm.S_0, K, T, R_D, R_F, KAPPA, ETA, SIGMA, RHO, Cm.V_0, lam, mu, sig)
    e1 = coarse(lam, mu, sig) - exact
    e2 = price(200, 100, 400, lam, mu, sig) - exact
    print("(%g, %g, %g): exact %.10f, error %.3e at 100x50x100, %.3e at 200x100x400, ratio %.2f" % (lam, mu, sig, exact, e1, e2, e1 / e2))
    assert abs(e1) <= 1.1e-2
    assert 3.0 * abs(e2) <= abs(e1)


@pytest.mark.parametrize("lam,mu,sig", JUMP_SETS, ids=IDS)
@pytest.mark.parametrize("mutation", ["no_compensator", "no_identity", "drop_half_var"])
def test_every_class_of_mistake_moves_the_price(mutation, lam, mu, sig):
    """Dropping the compensator term, dropping the -I, or mu_J where mu_J + sigma_J^2 / 2 belongs: each moves the 100x50x100
    price by more than 1e-2."""
    shift = abs(price(100, 50, 100, lam, mu, sig, **{mutation: True}) - coarse(lam, mu, sig))
    print("(%g, %g, %g) %s: %.3e" % (lam, mu, sig, mutation, shift))
    assert shift > 1e-2
