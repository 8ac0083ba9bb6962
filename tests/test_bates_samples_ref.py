"""What the Bates surface calls (hadi_bates_sample_ladder and its launchers) rest on, shown on the CPU reference
(tests/jumps_ref.py, tests/bates_samples_ref.py):

  homogeneity   jumps are multiplicative, so solving on the s-grid scaled by a = K' / K with the payoff scaled by a gives a U_K:
                the generator G = J - I - kbar diag(s) D depends on the grid through ratios only.  Within 1e-13 of max|U| (the
                level strike_samples states for plain Heston); with a = 2 the generators and the fields are bit-equal.
  ladder        calls with r_f = 0: the state after n steps of an N-step sweep is the n-step sweep (the sub-step of a step depends
                on delta_t only and sits at the end of the step), so a snapshot is the shorter call.
  accuracy      one surface value -- a strike read off the base grid through strike_samples -- against the semi-analytic Bates
                price, inside the 1.1e-2 that tests/test_jumps_ref.py records for the 100x50x100 grid.
"""
import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import bates_samples_ref as BS
import common as Cm
import jumps_ref as JR
from common import ETA, KAPPA, R_D, RHO, SIGMA, THETA, oracle_grids

K = 100.0
LAWS = [(0.5, -0.10, 0.15), (2.0, -0.05, 0.10), (0.3, 0.10, 0.30)]
IDS = ["lam%.1f_mu%+.2f_sig%.2f" % s for s in LAWS]
GRIDS = [(50, 25, 20), (100, 50, 40)]
SCALES = [0.8, 1.1, 1.25, 2.0]
R_F = 0.0

_base = {}


def solve(m1, m2, N, law, a=1.0, steps=None, U=None):
    """The field on the grid of K scaled by a (payoff scaled by a), after `steps` (default N) steps of delta_t = T / N."""
    vs, vv, ds, dv, U0 = (x[0] for x in oracle_grids(m1, m2, [K]))
    U_in = a * U0 if U is None else U
    return JR.solve_one(m1, m2, steps or N, Cm.T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, a * vs, vv, a * ds, dv, U_in, *law)


def base_field(m1, m2, N, law):
    if (m1, m2, N, law) not in _base:
        _base[(m1, m2, N, law)] = solve(m1, m2, N, law)
    return _base[(m1, m2, N, law)]


@pytest.mark.parametrize("law", LAWS, ids=IDS)
@pytest.mark.parametrize("m1,m2,N", GRIDS, ids=["50x25x20", "100x50x40"])
def test_homogeneity_under_jumps(m1, m2, N, law):
    U1 = base_field(m1, m2, N, law)
    top = np.abs(U1).max()
    vs = oracle_grids(m1, m2, [K])[0][0]
    for a in SCALES:
        Ua = solve(m1, m2, N, law, a)
        dev = np.abs(Ua - a * U1).max() / (a * top)
        print("%dx%dx%d %s a = %g: |U_aK - a U_K| / max|a U| = %.2e" % (m1, m2, N, law, a, dev))
        assert dev <= 1e-13
        if a == 2.0:
            assert np.array_equal(Ua, 2.0 * U1)
            assert np.array_equal(JR.generator(2.0 * vs, law[1], law[2]), JR.generator(vs, law[1], law[2]))


@pytest.mark.parametrize("law", LAWS[:2], ids=IDS[:2])
def test_a_snapshot_is_the_shorter_sweep(law):
    """8 steps = 3 steps, then 5 more from that state, bit for bit (calls, r_f = 0); and bates_samples_ref's snapshot q is the
    sample of the N = snap_steps[q] field by construction."""
    m1, m2, N = 50, 25, 8
    U3 = solve(m1, m2, N, law, steps=3)
    U8 = solve(m1, m2, N, law, steps=8)
    assert np.array_equal(solve(m1, m2, N, law, steps=5, U=U3), U8)
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [K])
    spots, scales = H.strike_samples(Cm.S_0, K, [90.0, 100.0, 110.0])
    vals, amp, top = BS.sample_ladder(m1, m2, [3, 8], Cm.T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U0, Cm.V_0, spots,
                                      scales, *law)
    assert vals.shape == (1, 2, 3) and top.shape == (1, 2)
    j0 = int(np.nonzero(np.abs(vv[0] - Cm.V_0) < 1e-10)[0][0])
    i0 = int(np.nonzero(np.abs(vs[0] - Cm.S_0) < 1e-10)[0][0])
    assert vals[0, 0, 1] == U3[j0 * (m1 + 1) + i0] and vals[0, 1, 1] == U8[j0 * (m1 + 1) + i0]  # (K' = K: the node of S_0, scale 1)


def test_a_surface_value_against_the_semi_analytic_price():
    m1, m2, N, law, strike = 100, 50, 100, LAWS[0], 110.0
    vs, vv, ds, dv, U0 = oracle_grids(m1, m2, [K])
    spots, scales = H.strike_samples(Cm.S_0, K, [strike])
    got = BS.sample_ladder(m1, m2, [N], Cm.T / N, THETA, R_D, R_F, RHO, SIGMA, KAPPA, ETA, vs, vv, ds, dv, U0, Cm.V_0, spots, scales,
                           *law)[0][0, 0, 0]
    exact = JR.bates_call_semi_analytic(Cm.S_0, strike, Cm.T, R_D, R_F, KAPPA, ETA, SIGMA, RHO, Cm.V_0, *law)
    print("K' = %g off the grid of K = %g: %.10f, semi-analytic %.10f, error %.3e" % (strike, K, got, exact, got - exact))
    assert abs(got - exact) <= 1.1e-2
