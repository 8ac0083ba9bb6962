"""Test-side reference of the Bates sample calls (hadi_bates_sample_ladder and its two launchers).  Nothing is defined here: snapshot
q is jumps_ref.solve_batch at N = snap_steps[q], and samples_ref.sample_batch on that field.  The Jacobian is nine (or six) such
calls on jumps8_ref's bumps.  TESTS ONLY.
"""
import numpy as np

import jumps8_ref as J8
import jumps_ref as JR
import samples_ref as SR
from oracle import oracle as O


def sample_ladder(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, V_0, spots, scales, lam, mu_j, sigma_j,
                  **kw):
    """(values, sum|w| |scale|, max|U|): [n][n_snap][n_samp] twice and [n][n_snap].  V_0: a scalar or [n] (the row that is sampled);
    kw goes to jumps_ref.solve_batch (dividends, put_strikes, scheme, dt_i, rows)."""
    n = vs.shape[0]
    vals, amps, tops = [], [], []
    for N in snaps:
        F = JR.solve_batch(m1, m2, int(N), dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, lam, mu_j, sigma_j, **kw)
        rows = kw.get("rows")
        if rows is not None:  # (the rows left out stay NaN: sample zeros there)
            F = np.where(np.isnan(F), 0.0, F)
        v, a, flags = SR.sample_batch(F, vs, vv, V_0, spots, scales)
        assert (flags == 0).all(), flags
        vals.append(v)
        amps.append(a)
        tops.append(np.abs(F).max(axis=1))
    return np.stack(vals, axis=1), np.stack(amps, axis=1), np.stack(tops, axis=1).reshape(n, len(snaps))


def base_samples(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, vs, ds, U, spots, scales, lam, mu_j, sigma_j, V_0_i=None,
                 **kw):
    """compute_base_prices_bates_samples: the v-grid rebuilt for V_0 (or V_0_i[k]), then sample_ladder on the row of that value."""
    n = vs.shape[0]
    v0 = np.array([V_0 if V_0_i is None else float(V_0_i[k]) for k in range(n)])
    Gv = [O.rebuild_variance(m2, v) for v in v0]
    vv, dv = np.stack([g[0] for g in Gv]), np.stack([g[1] for g in Gv])
    return sample_ladder(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, v0, spots, scales, lam, mu_j,
                         sigma_j, **kw)


def group_samples(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, vs, ds, U_0, spots, scales, lam, mu_j, sigma_j, n_par=8,
                  eps=1e-6, V_0_i=None, **kw):
    """(P [n_par + 1][n][n_snap][n_samp], sum|w| |scale| and max|U| of the base group): group 0 the base, then the bumped parameters
    in jumps8_ref.COLUMNS' order -- all nine groups for n_par = 8, the first six for n_par = 5."""
    assert n_par in (5, 8)
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    groups = [dict(), dict(kappa=kappa + eps), dict(eta=eta + eps), dict(sigma=sigma + eps), dict(rho=rho + eps),
              dict(V_0=V_0 + eps, V_0_i=v0i), dict(lam=J8._bump(lam, eps)), dict(mu_j=J8._bump(mu_j, eps)),
              dict(sigma_j=J8._bump(sigma_j, eps))][:n_par + 1]
    out, amp0, top0 = [], None, None
    for g in groups:
        a = dict(rho=rho, sigma=sigma, kappa=kappa, eta=eta, V_0=V_0, V_0_i=V_0_i, lam=lam, mu_j=mu_j, sigma_j=sigma_j)
        a.update(g)
        v, amp, top = base_samples(m1, m2, snaps, dt, theta, r_d, r_f, a["rho"], a["sigma"], a["kappa"], a["eta"], a["V_0"], vs, ds, U_0,
                                   spots, scales, a["lam"], a["mu_j"], a["sigma_j"], V_0_i=a["V_0_i"], **kw)
        out.append(v)
        if amp0 is None:
            amp0, top0 = amp, top
    return np.stack(out), amp0, top0


def jacobian(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, vs, ds, U_0, spots, scales, lam, mu_j, sigma_j, n_par=8,
             eps=1e-6, V_0_i=None, **kw):
    """(J [n][n_snap][n_samp][n_par], base [n][n_snap][n_samp], sum|w| |scale| of the base group): J[..., c] = (group c + 1 - base) / eps."""
    P, amp0, _ = group_samples(m1, m2, snaps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, vs, ds, U_0, spots, scales, lam, mu_j,
                               sigma_j, n_par=n_par, eps=eps, V_0_i=V_0_i, **kw)
    return np.moveaxis((P[1:] - P[0]) / eps, 0, -1).copy(), P[0], amp0


class RefSolver:
    """The two launchers of calibrate_bates_surface on this reference, for the LM loop; `calls` logs (name, n_par or 0), `last_amp`
    keeps sum|w| |scale| of the last Jacobian's samples."""

    def __init__(self):
        self.calls, self.last_amp = [], None

    def compute_jacobian_bates_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids,
                                       U_0, snap_steps, lam, mu, sig, shared_grid=False, jump_columns=False, scales=None, eps=1e-6,
                                       variant=0, dividends=None, **kw):
        n_par = 8 if jump_columns else 5
        self.calls.append(("jacobian", n_par))
        J, base, self.last_amp = jacobian(m1, m2, snap_steps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, grids.Vec_s, grids.Delta_s,
                                          np.asarray(U_0), spots, scales, lam, mu, sig, n_par=n_par, eps=eps)
        return J, base

    def compute_base_prices_bates_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids,
                                          ws, snap_steps, lam, mu, sig, shared_grid=False, scales=None, variant=0, dividends=None, **kw):
        self.calls.append(("base", 0))
        return base_samples(m1, m2, snap_steps, dt, theta, r_d, r_f, rho, sigma, kappa, eta, V_0, grids.Vec_s, grids.Delta_s,
                            np.asarray(ws.U), spots, scales, lam, mu, sig)[0]


# ---- the 6-strike x 3-maturity case of the surface loop: ONE 50x25 grid at K = 100, delta_t = 1 / 8, maturities of 2, 5 and 8 steps,
# calls with r_f = 0, a market made by this reference at the model of tests/common.py with the law (0.5, -0.10, 0.15) ----
LOOP_M1, LOOP_M2, LOOP_DT = 50, 25, 0.125
LOOP_BASE_STRIKE = 100.0
LOOP_STRIKES = (85.0, 92.0, 98.0, 103.0, 110.0, 118.0)
LOOP_MATURITIES = (0.25, 0.625, 1.0)
LOOP_LAW = (0.5, -0.10, 0.15)
LOOP_START_FACTORS = (1.1, 0.9, 1.1, 0.9, 1.0, 1.3, 1.2, 0.8)  # kappa, eta, sigma, rho, V_0, jump_intensity, jump_mean, jump_vol


def loop_case(H, Cm):
    """(grids, U_0, market [18], start [8]); H the package, Cm tests/common.py."""
    grids = H.GridViewsBatch.for_strikes(LOOP_M1, LOOP_M2, Cm.S_0, Cm.V_0, [LOOP_BASE_STRIKE])
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff([LOOP_BASE_STRIKE])
    spots, scales = H.strike_samples(Cm.S_0, LOOP_BASE_STRIKE, LOOP_STRIKES)
    snaps = [int(round(T / LOOP_DT)) for T in LOOP_MATURITIES]
    market = base_samples(LOOP_M1, LOOP_M2, snaps, LOOP_DT, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, Cm.V_0, grids.Vec_s,
                          grids.Delta_s, U0, spots, scales, *LOOP_LAW)[0].reshape(-1)
    truth = (Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0) + LOOP_LAW
    return grids, U0, market, tuple(t * f for t, f in zip(truth, LOOP_START_FACTORS))


def loop_run(H, Cm, solver, grids, U0, market, start, **kw):
    kw = dict(dict(max_iter=2, tol=1e-12, delta_tol=1e-12), **kw)
    return H.calibrate_bates_surface(solver, Cm.S_0, Cm.R_D, 0.0, *start[:5], LOOP_M1, LOOP_M2, Cm.THETA, LOOP_BASE_STRIKE, list(LOOP_STRIKES),
                                     list(LOOP_MATURITIES), LOOP_DT, grids, U0.copy(), market, *start[5:], **kw)
