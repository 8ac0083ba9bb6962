"""Test-side reference of a Bermudan sweep, built from oracle calls only (as scheme_ref.py is): operators A_k x and line
solves (I - theta dt A_k)^{-1} rhs from `oracle.operator`, the boundary vectors b, b1, b2 from the step-1 dump of
`oracle.solve`.  The time factor is exp(bc_rate dt n) with bc_rate = r_f for call data and -r_d for put data; the oracle's
dividend dating and jump are restated in numpy; then the projection U <- max(U, payoff) at the END of the listed steps.  The
Douglas step is written in the oracle's own evaluation order: without exercise steps the stepper reproduces `oracle.solve`
bit for bit (tests/test_bermudan_ref.py asserts it for EU and DIV, call and put).  The predictor-corrector schemes go through
the formulas of scheme_ref.py.

Step n is time to maturity n dt; n = N is the valuation date.  A dividend acts at the START of its step, exercise at the END.
"""
import math

import numpy as np

from oracle import oracle as O

DOUGLAS, CS, MCS, HV = 0, 1, 2, 3


def dividend_jump(vs, U, amount, pct, put, m1, m2):
    """device_solver.hpp:448-504 as the oracle restates it (heston_oracle.c, dividend_jump), one instance, field [m]."""
    Ut = U.reshape(m2 + 1, m1 + 1)
    out = np.empty_like(Ut)
    for i in range(m1 + 1):
        new_s = vs[i] * (1.0 - pct) - amount
        if new_s > 0:
            idx = 0
            for k in range(m1 + 1):  # first k with s[k] > new_s, 0 if none
                if vs[k] > new_s:
                    idx = k
                    break
            if idx > 0:
                s_low, s_high = vs[idx - 1], vs[idx]
                weight = (new_s - s_low) / (s_high - s_low)
                out[:, i] = (1.0 - weight) * Ut[:, idx - 1] + weight * Ut[:, idx]
            else:
                out[:, i] = Ut[:, 0]
        else:  # ex-dividend spot <= 0: a call is worth 0, a put its s = 0 value
            out[:, i] = Ut[:, 0] if put else 0.0
    return out.reshape(-1)


def dividend_steps(N, dt, dates):
    """The oracle's dating (heston_oracle.c, timestepping): {step n: index of the dividend paid at its start}."""
    paid, cur = {}, 0
    for n in range(1, N + 1):
        t, t_next = n * dt, (n + 1) * dt
        if cur < len(dates) and t <= dates[cur] and dates[cur] < t_next:
            paid[n] = cur
        if cur < len(dates) and t > dates[cur]:
            cur += 1
    return paid


def solve_one(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, ex_steps, payoff=None, dividends=None,
              put_strike=None, scheme=DOUGLAS):
    """One instance.  ex_steps: the steps at whose end U <- max(U, payoff) (zeros are padding); payoff: [m], default the
    initial U; dividends: (dates, amounts, percentages) or None; put_strike: the strike of put boundary data or None."""
    put = put_strike is not None
    p = O.make_params(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, O.EU,
                      option_type=O.PUT if put else O.CALL, strikes=put_strike)
    g = (vs, vv, ds, dv)
    U = np.array(U, dtype=np.float64).reshape(-1)
    pay = U.copy() if payoff is None else np.array(payoff, dtype=np.float64).reshape(-1)
    _, _, d = O.solve(p, *g, U, dump_step=1)  # same N as the run: the call's boundary data carry exp(-r_f dt (N - 1))
    b, b1, b2 = d["b"], d["b1"], d["b2"]
    b0 = b - b1 - b2
    A = lambda k, x: O.operator(p, k, *g, x)[0]
    solve = lambda k, rhs: O.operator(p, k, *g, rhs, b=rhs)[1]
    rate = -r_d if put else r_f
    ex = {int(n) for n in ex_steps if int(n) > 0}
    assert all(1 <= n <= N for n in ex)
    paid = dividend_steps(N, dt, dividends[0]) if dividends is not None else {}
    assert scheme == DOUGLAS or (not paid and not put)
    for n in range(1, N + 1):
        if n in paid:
            q = paid[n]
            U = dividend_jump(vs, U, dividends[1][q], dividends[2][q], put, m1, m2)
        A0U, A1U, A2U = A(0, U), A(1, U), A(2, U)
        e_n, e_nm1 = math.exp(rate * dt * n), math.exp(rate * dt * (n - 1))
        Y0 = U + dt * (A0U + A1U + A2U + b * e_nm1)
        Y1 = solve(1, Y0 + theta * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
        Y2 = solve(2, Y1 + theta * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
        if scheme == DOUGLAS:
            U = Y2
        else:
            A0Y2 = A(0, Y2)
            d0 = (A0Y2 + b0 * e_n) - (A0U + b0 * e_nm1)
            if scheme == CS:
                Yh = Y0 + 0.5 * dt * d0
            else:
                A1Y2, A2Y2 = A(1, Y2), A(2, Y2)
                dd = (A0Y2 + A1Y2 + A2Y2 + b * e_n) - (A0U + A1U + A2U + b * e_nm1)
                Yh = Y0 + theta * dt * d0 + (0.5 - theta) * dt * dd if scheme == MCS else Y0 + 0.5 * dt * dd
            if scheme == HV:
                Yt = solve(1, Yh - theta * dt * A1Y2)
                U = solve(2, Yt - theta * dt * A2Y2)
            else:
                Yt = solve(1, Yh + theta * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
                U = solve(2, Yt + theta * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
        if n in ex:
            U = np.maximum(U, pay)
    return U


def solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, ex_steps, payoff=None,
                dividends=None, put_strikes=None, scheme=DOUGLAS, N_i=None, dt_i=None, par_i=None, rows=None, models=None):
    """[n][m] fields, instance by instance.  ex_steps: one list for the batch or one list per instance; N_i / dt_i: per-instance
    step grids; par_i: {"rho_i": [...], ...} per-instance model parameters, or models: one (rho, sigma, kappa, eta) per
    instance; dividends: (dates, amounts, percentages) as tests/dividend_schedules.py builds them, dated on every instance's own
    step grid; rows: solve these instances only (the others stay NaN)."""
    n = vs.shape[0]
    ex = list(ex_steps)
    shared = not (ex and np.ndim(ex[0]) == 1)
    out = np.full((n, (m1 + 1) * (m2 + 1)), np.nan)
    par = par_i or {}
    assert models is None or (not par and len(models) == n)
    for k in (range(n) if rows is None else rows):
        pk = [par[key][k] if par.get(key) is not None else val
              for key, val in (("rho_i", rho), ("sigma_i", sigma), ("kappa_i", kappa), ("eta_i", eta))]
        if models is not None:
            pk = [float(x) for x in models[k]]
        out[k] = solve_one(m1, m2, int(N_i[k]) if N_i is not None else N, float(dt_i[k]) if dt_i is not None else dt, theta, r_d,
                           r_f, pk[0], pk[1], pk[2], pk[3], vs[k], vv[k], ds[k], dv[k], U[k], ex if shared else ex[k],
                           None if payoff is None else payoff[k], dividends,
                           None if put_strikes is None else float(put_strikes[k]), scheme)
    return out


def pick(vs, vv, U, S_0, V_0, m1):
    """The price pick of the launchers: first s-node within 1e-10 of S_0, first v-node within 1e-10 of V_0 (row 0 if none)."""
    i = int(np.nonzero(np.abs(vs - S_0) < 1e-10)[0][0])
    jj = np.nonzero(np.abs(vv - V_0) < 1e-10)[0]
    j = int(jj[0]) if len(jj) else 0
    return U[j * (m1 + 1) + i]


def base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U, ex_steps, V_0_i=None, **kw):
    """compute_base_prices_bermudan: the v-grid rebuilt for V_0 (or V_0_i[k]), the sweep, the pick.  Returns (prices, fields)."""
    n = vs.shape[0]
    v0 = [V_0 if V_0_i is None else float(V_0_i[k]) for k in range(n)]
    G = [O.rebuild_variance(m2, v) for v in v0]
    vv, dv = np.stack([g[0] for g in G]), np.stack([g[1] for g in G])
    F = solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, ex_steps, **kw)
    return np.array([pick(vs[k], vv[k], F[k], S_0, v0[k], m1) for k in range(n)]), F


def jacobian(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, ex_steps, eps=1e-6, V_0_i=None, **kw):
    """compute_jacobian_bermudan: six sweeps per instance (base, kappa, eta, sigma, rho + eps, V_0 + eps), J = (pert - base) / eps."""
    base, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, ex_steps, V_0_i=V_0_i, **kw)
    J = np.empty((vs.shape[0], 5))
    for col, (dk, de, dsg, dr) in enumerate(((eps, 0, 0, 0), (0, eps, 0, 0), (0, 0, eps, 0), (0, 0, 0, eps))):
        pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho + dr, sigma + dsg, kappa + dk, eta + de, S_0, V_0, vs, ds, U_0,
                              ex_steps, V_0_i=V_0_i, **kw)
        J[:, col] = (pert - base) / eps
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0 + eps, vs, ds, U_0, ex_steps, V_0_i=v0i, **kw)
    # (the pick of the perturbed solve looks for V_0 + eps: base_prices does, with the grid rebuilt for it)
    J[:, 4] = (pert - base) / eps
    return J, base
