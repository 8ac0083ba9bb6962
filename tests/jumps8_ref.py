"""Test-side reference of the eight-column Bates Jacobian (hadi_compute_jacobian_bates_jumps): nine calls of jumps_ref.base_prices
per batch, following the bump pattern of jumps_ref.jacobian -- base, then kappa, eta, sigma, rho + eps, V_0 + eps, and the three
jump parameters + eps, all forward differences with the one step eps.  A scalar jump parameter is bumped as a scalar, a
per-instance one per instance.
"""
import numpy as np

import jumps_ref as JR

COLUMNS = ("kappa", "eta", "sigma", "rho", "v0", "jump_intensity", "jump_mean", "jump_vol")


def _bump(x, eps):
    return np.asarray(x, dtype=np.float64) + eps if np.ndim(x) == 1 else float(x) + eps


def group_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, lam, mu_j, sigma_j, eps=1e-6,
                 V_0_i=None, **kw):
    """[9][n] prices and the nine [n][m] fields: group 0 the base, 1 .. 8 the bumped parameters in COLUMNS' order."""
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    groups = [
        dict(),
        dict(kappa=kappa + eps), dict(eta=eta + eps), dict(sigma=sigma + eps), dict(rho=rho + eps),
        dict(V_0=V_0 + eps, V_0_i=v0i),
        dict(lam=_bump(lam, eps)), dict(mu_j=_bump(mu_j, eps)), dict(sigma_j=_bump(sigma_j, eps)),
    ]
    prices, fields = [], []
    for g in groups:
        a = dict(rho=rho, sigma=sigma, kappa=kappa, eta=eta, V_0=V_0, V_0_i=V_0_i, lam=lam, mu_j=mu_j, sigma_j=sigma_j)
        a.update(g)
        p, F = JR.base_prices(m1, m2, N, dt, theta, r_d, r_f, a["rho"], a["sigma"], a["kappa"], a["eta"], S_0, a["V_0"], vs, ds, U_0,
                              a["lam"], a["mu_j"], a["sigma_j"], V_0_i=a["V_0_i"], **kw)
        prices.append(p)
        fields.append(F)
    return np.stack(prices), fields


def jacobian8(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, lam, mu_j, sigma_j, eps=1e-6,
              V_0_i=None, **kw):
    """(J [n][8], base [n]): J[:, c] = (price of group c + 1 - base) / eps."""
    P, _ = group_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, lam, mu_j, sigma_j, eps=eps,
                        V_0_i=V_0_i, **kw)
    return ((P[1:] - P[0]) / eps).T.copy(), P[0]


class RefSolver8:
    """The two launchers of calibrate_bates_jumps on this reference, for the LM loop."""

    @staticmethod
    def _a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U, law):
        return (m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, grids.Vec_s, grids.Delta_s, np.asarray(U)) + tuple(law)

    def compute_jacobian_bates_jumps(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, U_0,
                                     lam, mu, sig, shared_grid=False, eps=1e-6, **kw):
        return jacobian8(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U_0, (lam, mu, sig)), eps=eps)

    def compute_base_prices_bates(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, ws, lam,
                                  mu, sig, shared_grid=False, **kw):
        return JR.base_prices(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, ws.U, (lam, mu, sig)))[0]


# ---- the twelve-strike case of the eight-parameter LM loop: 50x25, N = 8, calls, a market made at the model of tests/common.py
# with the law (0.5, -0.10, 0.15); on the reference sum r^2 goes 4.2e-2 -> 6.4e-4 -> 1.0e-4 over two accepted steps ----
LOOP_M1, LOOP_M2, LOOP_N = 50, 25, 8
LOOP_STRIKES = (80.0, 83.0, 86.5, 90.0, 93.0, 97.5, 101.5, 105.5, 109.0, 113.0, 116.5, 120.0)
LOOP_LAW = (0.5, -0.10, 0.15)
LOOP_START_FACTORS = (1.1, 0.9, 1.1, 0.9, 1.0, 1.3, 1.2, 0.8)  # kappa, eta, sigma, rho, V_0, jump_intensity, jump_mean, jump_vol


def loop_case(H, Cm):
    """(grids, U_0, market, start [8]) of the case; H the package, Cm tests/common.py."""
    strikes = list(LOOP_STRIKES)
    grids = H.GridViewsBatch.for_strikes(LOOP_M1, LOOP_M2, Cm.S_0, Cm.V_0, strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(strikes)
    market = JR.base_prices(LOOP_M1, LOOP_M2, LOOP_N, Cm.T / LOOP_N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, Cm.S_0,
                            Cm.V_0, grids.Vec_s, grids.Delta_s, U0, *LOOP_LAW)[0]
    truth = (Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0) + LOOP_LAW
    return grids, U0, market, tuple(t * f for t, f in zip(truth, LOOP_START_FACTORS))


def loop_run(H, Cm, solver, grids, U0, market, start, **kw):
    return H.calibrate_bates_jumps(solver, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, *start[:5], LOOP_M1, LOOP_M2, LOOP_N, Cm.THETA, grids, U0.copy(),
                                   market, *start[5:], max_iter=2, tol=1e-12, **kw)
