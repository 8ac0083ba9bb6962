"""The generator of the jump term in 40-digit arithmetic (mpmath), row by row: the same definition as jumps_ref.generator and
hadi_jump_entry_value -- G = J - I - kbar diag(s) D, J[i][l] = E[phi_l(s_i Y)] -- evaluated on the fp64 grid taken exactly.  Phi
comes from mpmath's erfc on the side of the smaller tail, so a row's entries are good to about 1e-38 absolute, 25 orders below
what they are compared with.  CPU tests and the recorder of tests/golden/jump_exact_ill.json only: nothing on a GPU machine needs
mpmath."""
import numpy as np
from mpmath import mp, mpf

DPS = 40


def _phi_pair(d):
    """(Phi(d), 1 - Phi(d)) for an mpf, +-inf included."""
    if d == mp.inf:
        return mpf(1), mpf(0)
    if d == -mp.inf:
        return mpf(0), mpf(1)
    # one erfc, on the side of the smaller tail; the other side by subtraction from 1 (exact to 1e-40 absolute, which is all the
    # comparisons need: they are absolute, at 1e-13 times at most 1 / h <= 1e8)
    t = mp.erfc(abs(d) / mp.sqrt(2)) / 2
    return (1 - t, t) if d > 0 else (t, 1 - t)


def _dphi(p0, p1):
    """Phi(d1) - Phi(d0) from the two pairs, on the side of the smaller tail."""
    return p1[0] - p0[0] if p0[0] < p0[1] else p0[1] - p1[1]


def generator_rows(vs, mu, sigma, rows):
    """{i: [mpf] * (m1 + 1)} for the rows asked for (i >= 1)."""
    mp.dps = DPS
    s = [mpf(float(x)) for x in vs]
    m1 = len(s) - 1
    mu, sigma = mpf(float(mu)), mpf(float(sigma))
    kb = mp.exp(mu + sigma * sigma / 2) - 1
    h = [s[q + 1] - s[q] for q in range(m1)]
    out = {}
    for i in rows:
        assert 1 <= i <= m1
        si = s[i]
        # node x_l: d(x_l) and d(x_l) - sigma; x_0 counts as 0 (Phi = 0) where it is not positive, the last interval runs to infinity
        pa, pb = [], []
        for l in range(m1 + 1):
            if l == m1:
                d = mp.inf
            elif s[l] <= 0:
                d = -mp.inf
            else:
                d = (mp.log(s[l] / si) - mu) / sigma
            pa.append(_phi_pair(d))
            pb.append(_phi_pair(d - sigma if abs(d) != mp.inf else d))
        g = [mpf(0)] * (m1 + 1)
        for q in range(m1):  # interval [s_q, s_q+1): phi_q falls, phi_q+1 rises
            P0, P1 = _dphi(pa[q], pa[q + 1]), _dphi(pb[q], pb[q + 1])
            w = si * (1 + kb) * P1
            g[q] += (s[q + 1] * P0 - w) / h[q]
            g[q + 1] += (w - s[q] * P0) / h[q]
        g[i] -= 1
        if i < m1:
            a, b = h[i - 1], h[i]
            g[i - 1] -= kb * si * (-b / (a * (a + b)))
            g[i] -= kb * si * ((b - a) / (a * b))
            g[i + 1] -= kb * si * (a / (b * (a + b)))
        else:
            g[m1 - 1] -= kb * si * (-1 / h[m1 - 1])
            g[m1] -= kb * si * (1 / h[m1 - 1])
        out[i] = g
    return out


def as_float(row):
    return np.array([float(x) for x in row])


def action(row, u):
    """sum_l G[i][l] u[l] in 40 digits, rounded once."""
    mp.dps = DPS
    return float(mp.fsum(g * mpf(float(x)) for g, x in zip(row, u)))
