"""Test-side restatement of the four ADI time steppers (Douglas, Craig-Sneyd, Modified Craig-Sneyd, Hundsdorfer-Verwer)
built from oracle calls only: operators A_k x and line solves (I - theta dt A_k)^{-1} rhs from `oracle.operator`, the boundary
vectors b, b1, b2 from the step-1 dump of `oracle.solve` (b0 = b - b1 - b2).  Nothing under oracle/ knows MCS or HV; Douglas
and CS are written in the oracle's own evaluation order, so they reproduce `oracle.solve_batch` bit for bit.

With F_k(t, x) = A_k x + b_k e(t), e_n = exp(r_f dt n), F = F_0 + F_1 + F_2 (in 't Hout & Foulon):
    Y0 = U + dt F(t_{n-1}, U)
    Y1 = Y0 + theta dt (F1(t_n, Y1) - F1(t_{n-1}, U))            Y2 = Y1 + theta dt (F2(t_n, Y2) - F2(t_{n-1}, U))
    CS   Yh = Y0 + dt/2 (F0(t_n, Y2) - F0(t_{n-1}, U))
    MCS  Yh = Y0 + theta dt (F0(t_n, Y2) - F0(t_{n-1}, U)) + (1/2 - theta) dt (F(t_n, Y2) - F(t_{n-1}, U))
    HV   Yh = Y0 + dt/2 (F(t_n, Y2) - F(t_{n-1}, U))
    CS, MCS  the two implicit stages again against (t_{n-1}, U);  HV against (t_n, Y2).
"""
import math

import numpy as np

from oracle import oracle as O

DOUGLAS, CS, MCS, HV = 0, 1, 2, 3


class _Ops:
    def __init__(self, p, vs, vv, ds, dv, U0):
        self.p, self.g = p, (vs, vv, ds, dv)
        _, _, d = O.solve(p, vs, vv, ds, dv, U0, dump_step=1)  # same N as the run: the boundary data carry exp(-r_f dt (N - 1))
        self.b, self.b1, self.b2 = d["b"], d["b1"], d["b2"]
        self.b0 = self.b - self.b1 - self.b2

    def A(self, k, x):
        return O.operator(self.p, k, *self.g, x)[0]

    def solve(self, k, rhs):
        return O.operator(self.p, k, *self.g, rhs, b=rhs)[1]


def solve_one(p, vs, vv, ds, dv, U, scheme, theta=None):
    """One instance (European call, p.scheme ignored).  theta: the scheme's theta (default p.theta)."""
    theta = p.theta if theta is None else theta
    if theta != p.theta:
        p = O.make_params(p.m1, p.m2, p.N, p.delta_t, theta, p.r_d, p.r_f, p.rho, p.sigma, p.kappa, p.eta, O.EU)
    op = _Ops(p, vs, vv, ds, dv, U)
    b, b0, b1, b2 = op.b, op.b0, op.b1, op.b2
    dt, r_f = p.delta_t, p.r_f
    U = np.array(U, dtype=np.float64)
    for n in range(1, p.N + 1):
        A0U, A1U, A2U = op.A(0, U), op.A(1, U), op.A(2, U)
        e_n, e_nm1 = math.exp(r_f * dt * n), math.exp(r_f * dt * (n - 1))
        Y0 = U + dt * (A0U + A1U + A2U + b * e_nm1)
        Y1 = op.solve(1, Y0 + theta * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
        Y2 = op.solve(2, Y1 + theta * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
        if scheme == DOUGLAS:
            U = Y2
            continue
        A0Y2 = op.A(0, Y2)
        d0 = (A0Y2 + b0 * e_n) - (A0U + b0 * e_nm1)
        if scheme == CS:
            Yh = Y0 + 0.5 * dt * d0
        else:
            A1Y2, A2Y2 = op.A(1, Y2), op.A(2, Y2)
            d = (A0Y2 + A1Y2 + A2Y2 + b * e_n) - (A0U + A1U + A2U + b * e_nm1)
            if scheme == MCS:
                Yh = Y0 + theta * dt * d0 + (0.5 - theta) * dt * d
            else:
                Yh = Y0 + 0.5 * dt * d
        if scheme == HV:
            Yt = op.solve(1, Yh - theta * dt * A1Y2)
            U = op.solve(2, Yt - theta * dt * A2Y2)
        else:
            Yt = op.solve(1, Yh + theta * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
            U = op.solve(2, Yt + theta * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
    return U


def solve_batch(p, vs, vv, ds, dv, U, scheme, theta=None):
    """[n][m] fields, instance by instance."""
    return np.stack([solve_one(p, vs[k], vv[k], ds[k], dv[k], U[k], scheme, theta) for k in range(vs.shape[0])])


def time_error(U, Uref, vs, vv, m1, m2, s_lo=50.0, s_hi=150.0, v_hi=1.0):
    """max |U - Uref| over the nodes with s in [s_lo, s_hi] and v <= v_hi (one instance, fields [m])."""
    s = np.asarray(vs)
    v = np.asarray(vv)
    mask = ((s >= s_lo) & (s <= s_hi))[None, :] & (v <= v_hi)[:, None]
    diff = np.abs(np.asarray(U).reshape(m2 + 1, m1 + 1) - np.asarray(Uref).reshape(m2 + 1, m1 + 1))
    return float(diff[mask].max())
