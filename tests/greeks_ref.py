"""Test-side restatement of the Greeks contract of hadi_compute_greeks (include/hadi.h): three-point derivative operators on
the non-uniform axes as dense matrices, the eight ladder columns of one instance from a field in natural layout, and the
error bounds the tests hold the product to.  Theta is built from oracle calls only: A0 + A1 + A2 on U from `oracle.operator`,
the boundary vector b from the step-1 dump of `oracle.solve` -- the expression tests/scheme_ref.py uses for F.  Nothing here
calls the product."""
import math

import numpy as np

from oracle import oracle as O

PRICE, DELTA, GAMMA, DV, DVV, DSV, THETA, LAMBDA = range(8)
NAMES = ("price", "delta", "gamma", "dv", "dvv", "dsv", "theta", "lambda")
FIELD_EPS = 1e-10     # the project's field bound against the oracle on well-conditioned grids, x max|U|
ROUNDING_EPS = 1e-13  # same field, another summation order: ~30x the worst case 25 * 2^-53 * sum|w||U|


def node_weights(x, k):
    """(base, w1[3], w2[3]): first / second derivative at node k from the nodes base .. base + 2 (hadi.h)."""
    x = np.asarray(x, dtype=np.float64)
    m = len(x) - 1
    kc = min(max(k, 1), m - 1)
    a, b = x[kc] - x[kc - 1], x[kc + 1] - x[kc]
    w2 = np.array([2 / (a * (a + b)), -2 / (a * b), 2 / (b * (a + b))])
    if k == 0:
        w1 = np.array([-(2 * a + b) / (a * (a + b)), (a + b) / (a * b), -a / (b * (a + b))])
    elif k == m:
        w1 = np.array([b / (a * (a + b)), -(a + b) / (a * b), (a + 2 * b) / (b * (a + b))])
    else:
        w1 = np.array([-b / (a * (a + b)), (b - a) / (a * b), a / (b * (a + b))])
    return kc - 1, w1, w2


def _dense(x, which):
    n = len(x)
    M = np.zeros((n, n))
    for k in range(n):
        base, w1, w2 = node_weights(x, k)
        M[k, base:base + 3] = w1 if which == 1 else w2
    return M


def D1(x):
    """First derivative on the axis x as a dense matrix: interior beta weights, gamma at the first node, alpha at the last."""
    return _dense(x, 1)


def D2(x):
    """Second derivative: interior delta weights; an end node takes its interior neighbour's row."""
    return _dense(x, 2)


def find_node(x, x0):
    """First node within 1e-10 of x0 (the tolerance of the price pick), -1 if none."""
    hit = np.nonzero(np.abs(np.asarray(x) - x0) < 1e-10)[0]
    return int(hit[0]) if len(hit) else -1


def bc_rate(p):
    return -p.r_d if p.option_type == O.PUT else p.r_f


def boundary_vector(p, vs, vv, ds, dv, U_init, U_0=None):
    """b of the instance (step-1 dump of a run with the same N: the data carry exp(-r_f dt (N - 1))), plus that run's (U_T, lambda_bar_T)."""
    U, lam, d = O.solve(p, vs, vv, ds, dv, U_init, U_0, dump_step=1)
    return d["b"], U, lam


def rhs_F(p, vs, vv, ds, dv, U, lam, b):
    """F(t_N, U) = A0 U + A1 U + A2 U + b e_N + lambda_bar, the explicit right-hand side of the scheme; [m]."""
    e_N = math.exp(bc_rate(p) * p.delta_t * p.N)
    F = sum(O.operator(p, k, vs, vv, ds, dv, U)[0] for k in range(3)) + np.asarray(b) * e_N
    return F if lam is None else F + np.asarray(lam)


def ladder(p, vs, vv, ds, dv, U, lam, j0, b):
    """[m1+1][8]: the eight columns for every s-node of v-row j0.  U, lam (None for non-American variants) and b in natural
    layout [m]; p holds the instance's own parameters, N and delta_t."""
    m1, m2 = p.m1, p.m2
    Uf = np.asarray(U, dtype=np.float64).reshape(m2 + 1, m1 + 1)
    Ds1, Ds2, Dv1, Dv2 = D1(vs), D2(vs), D1(vv), D2(vv)
    out = np.zeros((m1 + 1, 8))
    out[:, PRICE] = Uf[j0]
    out[:, DELTA] = Ds1 @ Uf[j0]
    out[:, GAMMA] = Ds2 @ Uf[j0]
    out[:, DV] = Dv1[j0] @ Uf
    out[:, DVV] = Dv2[j0] @ Uf
    out[:, DSV] = Dv1[j0] @ (Uf @ Ds1.T)
    out[:, THETA] = -rhs_F(p, vs, vv, ds, dv, U, lam, b).reshape(m2 + 1, m1 + 1)[j0]
    if lam is not None:
        out[:, LAMBDA] = np.asarray(lam).reshape(m2 + 1, m1 + 1)[j0]
    return out


def stencil_norms(p, vs, vv, j0):
    """[m1+1][8]: W_G(i), the 1-norm of each column's stencil (price 1; dsv the product of the two 1-norms; theta the
    expression of the issue, factor 2 included; lambda 1 / dt)."""
    s = np.asarray(vs, dtype=np.float64)
    v = float(vv[j0])
    Wd, Wg = np.abs(D1(vs)).sum(axis=1), np.abs(D2(vs)).sum(axis=1)
    Wdv, Wdvv = float(np.abs(D1(vv)[j0]).sum()), float(np.abs(D2(vv)[j0]).sum())
    W = np.zeros((len(s), 8))
    W[:, PRICE] = 1.0
    W[:, DELTA] = Wd
    W[:, GAMMA] = Wg
    W[:, DV] = Wdv
    W[:, DVV] = Wdvv
    W[:, DSV] = Wd * Wdv
    W[:, THETA] = 2 * (p.r_d + 0.5 * v * s * s * Wg + abs(p.r_d - p.r_f) * s * Wd + 0.5 * p.sigma ** 2 * v * Wdvv +
                       p.kappa * abs(p.eta - v) * Wdv + abs(p.rho) * p.sigma * s * v * Wd * Wdv)
    W[:, LAMBDA] = 1.0 / p.delta_t
    return W


def propagated_bound(p, vs, vv, j0, umax):
    """Fields that agree within 1e-10 max|U|: |G - G_ref| <= 1e-10 max|U| W_G(i); [m1+1][8]."""
    return FIELD_EPS * umax * stencil_norms(p, vs, vv, j0)


def rounding_bound(p, vs, vv, j0, umax):
    """The SAME field through two evaluation orders: 1e-13 in place of 1e-10; price and lambda are copies -- bit-equal."""
    B = ROUNDING_EPS * umax * stencil_norms(p, vs, vv, j0)
    B[:, PRICE] = 0.0
    B[:, LAMBDA] = 0.0
    return B


def worst_ratio(got, ref, bound):
    """max over nodes and columns of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf), and where it is."""
    diff = np.abs(np.asarray(got) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, diff / bound)
    k = np.unravel_index(np.argmax(r), r.shape)
    return float(r[k]), k


def oracle_instances(m1, m2, strikes, Ns, dts, variant, put=False, r_f=0.007, models=None, V0=None, theta=None):
    """The oracle's run of every instance of a batch, each with its own strike, (N, dt) and model parameters
    (rho, sigma, kappa, eta): the shared grids and payoff [n][...] plus, per instance, the oracle's parameter block, U_T,
    lambda_bar_T (None unless American) and boundary vector b."""
    import common as Cm
    n = len(strikes)
    V0 = Cm.V_0 if V0 is None else V0
    theta = Cm.THETA if theta is None else theta
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes, V0)
    if put:
        U0 = Cm.put_payoff(vs, strikes, m2)
    v = Cm.VARIANT[variant] if isinstance(variant, str) else variant
    inst = []
    for k in range(n):
        model = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA) if models is None else tuple(models[k])
        p = O.make_params(m1, m2, int(Ns[k]), float(dts[k]), theta, Cm.R_D, r_f, *model, v,
                          Cm.DIVS if v in (O.DIV, O.AM_DIV) else None, option_type=O.PUT if put else O.CALL,
                          strikes=[strikes[k]] if put else None)
        b, U, lam = boundary_vector(p, vs[k], vv[k], ds[k], dv[k], U0[k], U0[k] if v in (O.AM, O.AM_DIV) else None)
        inst.append({"p": p, "U": U, "lam": lam, "b": b})
    return vs, vv, ds, dv, U0, inst
