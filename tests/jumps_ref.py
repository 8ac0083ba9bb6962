"""Test-side reference of a Bates sweep (Heston plus compound-Poisson lognormal jumps in the spot), built from oracle calls and
numpy: the stepper of barrier_ref.solve_one (operators and line solves from `oracle.operator`, the boundary vectors from the
step-1 dump of `oracle.solve`, the oracle's dividend dating and jump restated in numpy, the four schemes in the oracle's own
evaluation order) with the jump sub-step at the END of every step:

    U_row <- U_row + a (G U_row),   a = lambda dt,   on every v-row,

G = J - I - kbar diag(s) D the generator of the jump term on the instance's own s-grid (generator() below), row 0 all zero.
With lambda = 0 the sub-step is not taken and the stepper reproduces `oracle.solve` bit for bit (tests/test_jumps_ref.py asserts
it for EU and DIV, call and put).  The splitting is first order in time; the boundary data stay the vanilla option's.

bates_call_semi_analytic is the characteristic-function price of a European call: Heston's "little trap" form with the drift
r_d - r_f - lambda kbar, times the Merton jump factor.
"""
import math

import numpy as np
from scipy.integrate import quad
from scipy.special import ndtr

import bermudan_ref as BR
from oracle import oracle as O

DOUGLAS, CS, MCS, HV = BR.DOUGLAS, BR.CS, BR.MCS, BR.HV


def kbar(mu, sigma, drop_half_var=False):
    """E[Y] - 1 for ln Y ~ N(mu, sigma^2).  drop_half_var=True is the MUTATION `mu` for `mu + sigma^2 / 2`."""
    return math.exp(mu if drop_half_var else mu + 0.5 * sigma * sigma) - 1.0


def _dphi(d0, d1):
    """Phi(d1) - Phi(d0) for d0 <= d1, taken on the side of the smaller tail (no cancellation against 1)."""
    return np.where(d0 > 0.0, ndtr(-d0) - ndtr(-d1), ndtr(d1) - ndtr(d0))


def expectation_matrix(vs, mu, sigma, kb=None):
    """J [m1+1][m1+1]: J[i][l] = E[phi_l(s_i Y)], phi_l the hat functions of the piecewise-linear interpolant on vs, the last
    interval's two linear pieces continued beyond s_max.  Row 0 (s = 0) is left zero."""
    vs = np.asarray(vs, dtype=np.float64)
    m1 = vs.size - 1
    kb = kbar(mu, sigma) if kb is None else kb
    J = np.zeros((m1 + 1, m1 + 1))
    si = vs[1:]

    def d(x):  # Phi(d(0)) = 0, Phi(d(inf)) = 1
        if x <= 0.0 or np.isinf(x):
            return np.full(si.shape, -np.inf if x <= 0.0 else np.inf)
        return (np.log(x / si) - mu) / sigma

    for q in range(m1):  # interval [s_q, s_q+1), the last one up to infinity
        x0, x1 = vs[q], (vs[q + 1] if q < m1 - 1 else np.inf)
        h = vs[q + 1] - vs[q]
        d0, d1 = d(x0), d(x1)
        P0, P1 = _dphi(d0, d1), _dphi(d0 - sigma, d1 - sigma)
        # phi_q falls: (s_q+1 - x) / h;  phi_q+1 rises: (x - s_q) / h
        J[1:, q] += (vs[q + 1] / h) * P0 + (-1.0 / h) * si * (1.0 + kb) * P1
        J[1:, q + 1] += (-vs[q] / h) * P0 + (1.0 / h) * si * (1.0 + kb) * P1
    return J


def derivative_matrix(vs):
    """D [m1+1][m1+1]: the three-point central first-derivative stencil on the non-uniform grid (the weights of hadi_fd_beta) for
    0 < i < m1, the two-point backward difference at i = m1; row 0 zero."""
    vs = np.asarray(vs, dtype=np.float64)
    m1 = vs.size - 1
    h = np.diff(vs)
    D = np.zeros((m1 + 1, m1 + 1))
    for i in range(1, m1):
        a, b = h[i - 1], h[i]
        D[i, i - 1] = -b / (a * (a + b))
        D[i, i] = (b - a) / (a * b)
        D[i, i + 1] = a / (b * (a + b))
    D[m1, m1 - 1], D[m1, m1] = -1.0 / h[m1 - 1], 1.0 / h[m1 - 1]
    return D


def generator(vs, mu, sigma, no_compensator=False, no_identity=False, drop_half_var=False):
    """G = J - I - kbar diag(s) D on the grid vs, natural order, row 0 all zero.  The three flags are the MUTATIONS of
    test_jumps_ref.py."""
    vs = np.asarray(vs, dtype=np.float64)
    kb = kbar(mu, sigma, drop_half_var)
    G = expectation_matrix(vs, mu, sigma, kb)
    if not no_identity:
        G -= np.eye(vs.size)
    if not no_compensator:
        G -= kb * vs[:, None] * derivative_matrix(vs)
    G[0, :] = 0.0
    return G


def jump_substep(U, G, a, m1, m2):
    """U <- U + a (G U) on every v-row of the natural field [(m2+1)(m1+1)]."""
    F = U.reshape(m2 + 1, m1 + 1)
    return (F + a * (F @ G.T)).reshape(-1)


def solve_one(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, lam=0.0, mu_j=0.0, sigma_j=0.1,
              dividends=None, put_strike=None, scheme=DOUGLAS, G=None, **mut):
    """One instance.  lam, mu_j, sigma_j: the jump law; dividends: (dates, amounts, percentages) or None; put_strike: the strike
    of put boundary data or None; G: a generator built elsewhere (shared), else generator(vs, mu_j, sigma_j, **mut)."""
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
    a = lam * dt
    assert 0.0 <= a <= 1.0
    if a != 0.0 and G is None:
        G = generator(vs, mu_j, sigma_j, **mut)
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
        if a != 0.0:
            U = jump_substep(U, G, a, m1, m2)
    return U


def per_instance(x, k):
    """Entry k of a scalar or a sequence."""
    return float(x[k]) if np.ndim(x) == 1 else float(x)


def solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, lam, mu_j, sigma_j, dividends=None,
                put_strikes=None, scheme=DOUGLAS, N_i=None, dt_i=None, rows=None, models=None):
    """[n][m] fields, instance by instance.  lam / mu_j / sigma_j: a scalar or one value per instance; N_i / dt_i: per-instance
    step grids; models: one (rho, sigma, kappa, eta) per instance; dividends: (dates, amounts, percentages), dated on every
    instance's own step grid; rows: solve these instances only (the others stay NaN)."""
    n = vs.shape[0]
    out = np.full((n, (m1 + 1) * (m2 + 1)), np.nan)
    assert models is None or len(models) == n
    for k in (range(n) if rows is None else rows):
        mk = (rho, sigma, kappa, eta) if models is None else tuple(float(x) for x in models[k])
        out[k] = solve_one(m1, m2, int(N_i[k]) if N_i is not None else N, float(dt_i[k]) if dt_i is not None else dt, theta, r_d,
                           r_f, *mk, vs[k], vv[k], ds[k], dv[k], U[k], per_instance(lam, k), per_instance(mu_j, k),
                           per_instance(sigma_j, k), dividends, None if put_strikes is None else float(put_strikes[k]), scheme)
    return out


def base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U, lam, mu_j, sigma_j, V_0_i=None, **kw):
    """compute_base_prices_bates: the v-grid rebuilt for V_0 (or V_0_i[k]), the sweep, the pick.  Returns (prices, fields)."""
    n = vs.shape[0]
    v0 = [V_0 if V_0_i is None else float(V_0_i[k]) for k in range(n)]
    Gv = [O.rebuild_variance(m2, v) for v in v0]
    vv, dv = np.stack([g[0] for g in Gv]), np.stack([g[1] for g in Gv])
    F = solve_batch(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, vs, vv, ds, dv, U, lam, mu_j, sigma_j, **kw)
    return np.array([BR.pick(vs[k], vv[k], F[k], S_0, v0[k], m1) for k in range(n)]), F


def jacobian(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, lam, mu_j, sigma_j, eps=1e-6,
             V_0_i=None, **kw):
    """compute_jacobian_bates: six sweeps per instance (base, kappa, eta, sigma, rho + eps, V_0 + eps), J = (pert - base) / eps;
    the jump parameters are held fixed."""
    jp = (lam, mu_j, sigma_j)
    base, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, vs, ds, U_0, *jp, V_0_i=V_0_i, **kw)
    J = np.empty((vs.shape[0], 5))
    for col, (dk, de, dsg, dr) in enumerate(((eps, 0, 0, 0), (0, eps, 0, 0), (0, 0, eps, 0), (0, 0, 0, eps))):
        pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho + dr, sigma + dsg, kappa + dk, eta + de, S_0, V_0, vs, ds, U_0,
                              *jp, V_0_i=V_0_i, **kw)
        J[:, col] = (pert - base) / eps
    v0i = None if V_0_i is None else np.asarray(V_0_i) + eps
    pert, _ = base_prices(m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0 + eps, vs, ds, U_0, *jp, V_0_i=v0i, **kw)
    J[:, 4] = (pert - base) / eps
    return J, base


def bates_call_semi_analytic(S0, K, T, r_d, r_f, kappa, eta, sigma, rho, v0, lam, mu_j, sigma_j):
    """Bates (1996) European call by Gil-Pelaez inversion: Heston's characteristic function ("little trap" form, as in
    tests/test_reference_pins.py) with the drift r_d - r_f - lambda kbar, times exp(lambda T (exp(i u mu_J - sigma_J^2 u^2 / 2) - 1))."""
    kb = kbar(mu_j, sigma_j)

    def cf(u):
        x = np.log(S0) + (r_d - r_f - lam * kb) * T
        d = np.sqrt((rho * sigma * 1j * u - kappa) ** 2 + sigma ** 2 * (1j * u + u * u))
        g = (kappa - rho * sigma * 1j * u - d) / (kappa - rho * sigma * 1j * u + d)
        C = kappa * eta / sigma ** 2 * ((kappa - rho * sigma * 1j * u - d) * T - 2 * np.log((1 - g * np.exp(-d * T)) / (1 - g)))
        D = (kappa - rho * sigma * 1j * u - d) / sigma ** 2 * (1 - np.exp(-d * T)) / (1 - g * np.exp(-d * T))
        return np.exp(1j * u * x + C + D * v0 + lam * T * (np.exp(1j * u * mu_j - 0.5 * sigma_j ** 2 * u * u) - 1.0))
    k = np.log(K)
    kw = dict(limit=2000, epsabs=1e-13, epsrel=1e-13)
    P1 = 0.5 + quad(lambda u: (np.exp(-1j * u * k) * cf(u - 1j) / (1j * u * cf(-1j))).real, 1e-12, 400, **kw)[0] / np.pi
    P2 = 0.5 + quad(lambda u: (np.exp(-1j * u * k) * cf(u) / (1j * u)).real, 1e-12, 400, **kw)[0] / np.pi
    return S0 * np.exp(-r_f * T) * P1 - K * np.exp(-r_d * T) * P2
