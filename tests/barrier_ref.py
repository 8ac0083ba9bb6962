"""Test-side reference of a discretely monitored knock-out sweep, built from oracle calls only: the stepper of
bermudan_ref.solve_one (operators and line solves from `oracle.operator`, the boundary vectors from the step-1 dump of
`oracle.solve`, the oracle's dividend dating and jump restated in numpy, the Douglas step in the oracle's own evaluation order)
with the knock-out in place of the projection: at the END of every listed step, U <- rebate on every node whose spot satisfies
s_i <= lower or s_i >= upper, in every v-row.  Without monitoring steps the stepper reproduces `oracle.solve` bit for bit
(tests/test_barrier_ref.py asserts it for EU and DIV, call and put).

Step n is time to maturity n dt; n = N is the valuation date.  A dividend acts at the START of its step, the barrier at its END.
The rebate is not discounted; the boundary data stay the vanilla option's.
"""
import math

import numpy as np

import bermudan_ref as BR
from oracle import oracle as O

DOUGLAS, CS, MCS, HV = BR.DOUGLAS, BR.CS, BR.MCS, BR.HV


def knocked_nodes(vs, lower, upper, strict=False):
    """[m1+1] bool: touching knocks out.  strict=True is the MUTATION `<` for `<=` (and `>` for `>=`) of test_barrier_ref.py."""
    lo = -np.inf if lower is None else lower
    up = np.inf if upper is None else upper
    return ((vs < lo) | (vs > up)) if strict else ((vs <= lo) | (vs >= up))


def knock(U, knocked, rebate, m1, m2):
    out = U.reshape(m2 + 1, m1 + 1).copy()
    out[:, knocked] = rebate
    return out.reshape(-1)


def solve_one(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, mon_steps, lower=None, upper=None, rebate=0.0,
              dividends=None, put_strike=None, scheme=DOUGLAS, strict=False):
    """One instance.  mon_steps: the steps at whose end the knock-out acts (zeros are padding); lower / upper: None = no barrier
    on that side; dividends: (dates, amounts, percentages) or None; put_strike: the strike of put boundary data or None."""
    put = put_strike is not None
    p = O.make_params(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, O.EU,
                      option_type=O.PUT if put else O.CALL, strikes=put_strike)
    g = (vs, vv, ds, dv)
    U = np.array(U, dtype=np.float64).reshape(-1)
    _, _, d = O.solve(p, *g, U, dump_step=1)  # same N as the run: the call's boundary data carry exp(-r_f dt (N - 1))
    b, b1, b2 = d["b"], d["b1"], d["b2"]
    b0 = b - b1 - b2
    A = lambda k, x: O.operator(p, k, *g, x)[0]
    solve = lambda k, rhs: O.operator(p, k, *g, rhs, b=rhs)[1]
    rate = -r_d if put else r_f
    mon = {int(n) for n in mon_steps if int(n) > 0}
    assert all(1 <= n <= N for n in mon)
    knocked = knocked_nodes(np.asarray(vs, dtype=np.float64), lower, upper, strict)
    paid = BR.dividend_steps(N, dt, dividends[0]) if dividends is not None else {}
    assert scheme == DOUGLAS or (not paid and not put)
    for n in range(1, N + 1):
        if n in paid:
            q = paid[n]
            U = BR.dividend_jump(vs, U, dividends[1][q], dividends[2][q], put, m1, m2)
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
        if n in mon:
            U = knock(U, knocked, rebate, m1, m2)
    return U


def per_instance(x, k, default):
    """Entry k of a scalar, a sequence or None."""
    if x is None:
        return default
    return float(x[k]) if np.ndim(x) == 1 else float(x)


def solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, mon_steps, lower=None, upper=None,
                rebate=None, dividends=None, put_strikes=None, scheme=DOUGLAS, N_i=None, dt_i=None, rows=None, models=None):
    """[n][m] fields, instance by instance.  mon_steps: one list for the batch or one list per instance; lower / upper / rebate:
    a scalar, one value per instance, or None; N_i / dt_i: per-instance step grids; models: one (rho, sigma, kappa, eta) per
    instance; dividends: (dates, amounts, percentages) as tests/dividend_schedules.py builds them, dated on every instance's own
    step grid; rows: solve these instances only (the others stay NaN)."""
    n = vs.shape[0]
    mon = list(mon_steps)
    shared = not (mon and np.ndim(mon[0]) == 1)
    out = np.full((n, (m1 + 1) * (m2 + 1)), np.nan)
    assert models is None or len(models) == n
    for k in (range(n) if rows is None else rows):
        mk = (rho, sigma, kappa, eta) if models is None else tuple(float(x) for x in models[k])
        out[k] = solve_one(m1, m2, int(N_i[k]) if N_i is not None else N, float(dt_i[k]) if dt_i is not None else dt, theta, r_d,
                           r_f, *mk, vs[k], vv[k], ds[k], dv[k], U[k], mon if shared else mon[k],
                           per_instance(lower, k, None), per_instance(upper, k, None), per_instance(rebate, k, 0.0), dividends,
                           None if put_strikes is None else float(put_strikes[k]), scheme)
    return out


def base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U, mon_steps, V_0_i=None, **kw):
    """compute_base_prices_barrier: the v-grid rebuilt for V_0 (or V_0_i[k]), the sweep, the pick.  Returns (prices, fields)."""
    n = vs.shape[0]
    v0 = [V_0 if V_0_i is None else float(V_0_i[k]) for k in range(n)]
    G = [O.rebuild_variance(m2, v) for v in v0]
    vv, dv = np.stack([g[0] for g in G]), np.stack([g[1] for g in G])
    F = solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, mon_steps, **kw)
    return np.array([BR.pick(vs[k], vv[k], F[k], S_0, v0[k], m1) for k in range(n)]), F


def jacobian(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, mon_steps, eps=1e-6, V_0_i=None, **kw):
    """compute_jacobian_barrier: six sweeps per instance (base, kappa, eta, sigma, rho + eps, V_0 + eps), J = (pert - base) / eps."""
    base, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, mon_steps, V_0_i=V_0_i, **kw)
    J = np.empty((vs.shape[0], 5))
    for col, (dk, de, dsg, dr) in enumerate(((eps, 0, 0, 0), (0, eps, 0, 0), (0, 0, eps, 0), (0, 0, 0, eps))):
        pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho + dr, sigma + dsg, kappa + dk, eta + de, S_0, V_0, vs, ds, U_0,
                              mon_steps, V_0_i=V_0_i, **kw)
        J[:, col] = (pert - base) / eps
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0 + eps, vs, ds, U_0, mon_steps, V_0_i=v0i, **kw)
    J[:, 4] = (pert - base) / eps
    return J, base
