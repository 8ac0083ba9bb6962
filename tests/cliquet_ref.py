"""Test-side reference of a sweep with strike fixings (forward-start options, cliquets), built from oracle calls only: the stepper
of barrier_ref.solve_one (operators and line solves from `oracle.operator`, the boundary vectors from the step-1 dump of
`oracle.solve`, the oracle's dividend dating and jump restated in numpy, the Douglas step in the oracle's own evaluation order)
with the fixing in place of the knock-out: at the END of every listed step, on every v-row j,

    c_j     = U(i_ref, j)
    U(i, j) <- a_i * c_j + w * P(i, j)      (the term w * P only when w != 0)

with a_i = s_i / s_{i_ref} (SHARES; exactly 1 at i_ref) or 1 (RETURN).  Without fixings the stepper reproduces `oracle.solve` bit
for bit (tests/test_cliquet_ref.py asserts it for EU and DIV, call and put).

Step n is time to maturity n dt; n = N is the valuation date.  A dividend acts at the START of its step, the fixing at its END.
The boundary data stay the vanilla option's.
"""
import math

import numpy as np

import bermudan_ref as BR
from oracle import oracle as O

DOUGLAS, CS, MCS, HV = BR.DOUGLAS, BR.CS, BR.MCS, BR.HV
SHARES, RETURN = 0, 1


def find_node(vs, spot):
    """The price pick's rule: the first node within 1e-10, or -1."""
    hit = np.nonzero(np.abs(np.asarray(vs, dtype=np.float64) - spot) < 1e-10)[0]
    return int(hit[0]) if hit.size else -1


def fixing(U, vs, i_ref, mode, w, P, m1, m2):
    """The event on one field [(m2+1)(m1+1)]."""
    F = U.reshape(m2 + 1, m1 + 1)
    c = F[:, i_ref].copy()
    if mode == RETURN:
        out = np.repeat(c[:, None], m1 + 1, axis=1)
    else:
        a = np.asarray(vs, dtype=np.float64) / vs[i_ref]
        out = a[None, :] * c[:, None]
        out[:, i_ref] = c
    if w != 0.0:
        out = out + w * P.reshape(m2 + 1, m1 + 1)
    return out.reshape(-1)


def solve_one(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, fix_steps, ref_spot=None, mode=SHARES,
              weights=None, payoff=None, dividends=None, put_strike=None, scheme=DOUGLAS, i_ref=None):
    """One instance.  fix_steps: the steps at whose end the fixing acts (zeros are padding); weights: parallel to fix_steps or
    None (= 0); payoff: P, None = the initial U; i_ref: overrides the node of ref_spot (the MUTATIONS of test_cliquet_ref.py);
    dividends: (dates, amounts, percentages) or None; put_strike: the strike of put boundary data or None."""
    put = put_strike is not None
    p = O.make_params(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, O.EU,
                      option_type=O.PUT if put else O.CALL, strikes=put_strike)
    g = (vs, vv, ds, dv)
    U = np.array(U, dtype=np.float64).reshape(-1)
    P = U.copy() if payoff is None else np.array(payoff, dtype=np.float64).reshape(-1)
    _, _, d = O.solve(p, *g, U, dump_step=1)  # same N as the run: the call's boundary data carry exp(-r_f dt (N - 1))
    b, b1, b2 = d["b"], d["b1"], d["b2"]
    b0 = b - b1 - b2
    A = lambda k, x: O.operator(p, k, *g, x)[0]
    solve = lambda k, rhs: O.operator(p, k, *g, rhs, b=rhs)[1]
    rate = -r_d if put else r_f
    fix = {}
    for q, n in enumerate(fix_steps):
        if int(n) > 0:
            fix[int(n)] = 0.0 if weights is None else float(weights[q])
    assert all(1 <= n <= N for n in fix)
    if fix and i_ref is None:
        i_ref = find_node(vs, ref_spot)
        assert i_ref >= 0, "ref_spot is not a node"
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
        if n in fix:
            U = fixing(U, vs, i_ref, mode, fix[n], P, m1, m2)
    return U


def per_instance(x, k, default):
    """Entry k of a scalar, a sequence or None."""
    if x is None:
        return default
    return x[k] if np.ndim(x) == 1 else x


def solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, fix_steps, ref_spot=None, mode=SHARES,
                weights=None, payoff=None, dividends=None, put_strikes=None, scheme=DOUGLAS, N_i=None, dt_i=None, rows=None,
                models=None):
    """[n][m] fields, instance by instance.  fix_steps: one list for the batch or one list per instance, and weights likewise
    (parallel to it) or None; ref_spot / mode: a scalar or one value per instance; payoff: [n][m] or None (the initial U);
    N_i / dt_i: per-instance step grids; models: one (rho, sigma, kappa, eta) per instance; rows: solve these instances only."""
    n = vs.shape[0]
    fix = list(fix_steps)
    shared = not (fix and np.ndim(fix[0]) == 1)
    out = np.full((n, (m1 + 1) * (m2 + 1)), np.nan)
    assert models is None or len(models) == n
    for k in (range(n) if rows is None else rows):
        mk = (rho, sigma, kappa, eta) if models is None else tuple(float(x) for x in models[k])
        wk = None if weights is None else (weights if shared else weights[k])
        out[k] = solve_one(m1, m2, int(N_i[k]) if N_i is not None else N, float(dt_i[k]) if dt_i is not None else dt, theta, r_d,
                           r_f, *mk, vs[k], vv[k], ds[k], dv[k], U[k], fix if shared else fix[k],
                           float(per_instance(ref_spot, k, np.nan)), int(per_instance(mode, k, SHARES)), wk,
                           None if payoff is None else payoff[k], dividends,
                           None if put_strikes is None else float(put_strikes[k]), scheme)
    return out


def base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U, fix_steps, V_0_i=None, **kw):
    """compute_base_prices_cliquet: the v-grid rebuilt for V_0 (or V_0_i[k]), the sweep, the pick.  Returns (prices, fields)."""
    n = vs.shape[0]
    v0 = [V_0 if V_0_i is None else float(V_0_i[k]) for k in range(n)]
    G = [O.rebuild_variance(m2, v) for v in v0]
    vv, dv = np.stack([g[0] for g in G]), np.stack([g[1] for g in G])
    F = solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, fix_steps, **kw)
    return np.array([BR.pick(vs[k], vv[k], F[k], S_0, v0[k], m1) for k in range(n)]), F


def jacobian(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, fix_steps, eps=1e-6, V_0_i=None, **kw):
    """compute_jacobian_cliquet: six sweeps per instance (base, kappa, eta, sigma, rho + eps, V_0 + eps), J = (pert - base) / eps."""
    base, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, fix_steps, V_0_i=V_0_i, **kw)
    J = np.empty((vs.shape[0], 5))
    for col, (dk, de, dsg, dr) in enumerate(((eps, 0, 0, 0), (0, eps, 0, 0), (0, 0, eps, 0), (0, 0, 0, eps))):
        pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho + dr, sigma + dsg, kappa + dk, eta + de, S_0, V_0, vs, ds, U_0,
                              fix_steps, V_0_i=V_0_i, **kw)
        J[:, col] = (pert - base) / eps
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0 + eps, vs, ds, U_0, fix_steps, V_0_i=v0i, **kw)
    J[:, 4] = (pert - base) / eps
    return J, base
