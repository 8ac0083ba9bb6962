"""numpy reference of the sampled ladder (hadi_sample_ladder, include/hadi.h): taps and weights from the definition, applied to
fields in natural order U[i + j (m1 + 1)].  TESTS ONLY.

For one instance: row j0 = the first v-node within 1e-10 of V_0 (row 0 if none); with s_0 < .. < s_m1 and the spot x
  node hit    the first i with |s_i - x| < 1e-10: one tap of weight 1
  off grid    x NaN, x < s_0 or x > s_m1 (no node hit): NaN, flag OFF_GRID
  interior    i = largest index with s_i < x, i0 = min(max(i - 1, 0), m1 - 3), w_a = prod_{b != a}(x - s_{i0+b}) /
              prod_{b != a}(s_{i0+a} - s_{i0+b}), both products over increasing b, one division
  degenerate  a non-finite weight: NaN, flag DEGENERATE
value = (((w0 U0) + w1 U1) + w2 U2) + w3 U3, times the scale (the library fuses the three additions; the difference is round-off
far below the bound 1e-10 sum|w| |scale| max|U| the tests use)."""
import numpy as np

TOL = 1e-10
OFF_GRID, DEGENERATE = 1, 2


def row_index(vec_v, V_0):
    hit = np.nonzero(np.abs(np.asarray(vec_v) - V_0) < TOL)[0]
    return int(hit[0]) if hit.size else 0


def taps(vec_s, x):
    """(indices [4], weights [4], flag) of one spot on one s-grid; a node hit is the node four times with weights 1, 0, 0, 0."""
    s = np.asarray(vec_s, dtype=np.float64)
    m1 = s.size - 1
    hit = np.nonzero(np.abs(s - x) < TOL)[0]
    if hit.size:
        return np.full(4, int(hit[0])), np.array([1.0, 0.0, 0.0, 0.0]), 0
    if not (x >= s[0]) or not (x <= s[m1]):
        return np.full(4, -1), np.zeros(4), OFF_GRID
    if m1 < 3:
        return np.full(4, -1), np.zeros(4), DEGENERATE
    i = int(np.nonzero(s < x)[0][-1])
    i0 = min(max(i - 1, 0), m1 - 3)
    w = np.empty(4)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(4):
            num, den = np.float64(1.0), np.float64(1.0)
            for b in range(4):
                if b != a:
                    num = num * (x - s[i0 + b])
                    den = den * (s[i0 + a] - s[i0 + b])
            w[a] = num / den
    if not np.isfinite(w).all():
        return np.full(4, -1), np.zeros(4), DEGENERATE
    return np.arange(i0, i0 + 4), w, 0


def sample_field(U, vec_s, vec_v, V_0, spots, scales=None):
    """One instance: (values [n_samp], sum|w| |scale| [n_samp], flags [n_samp]) of a field U [m] in natural order."""
    s = np.asarray(vec_s, dtype=np.float64)
    m1 = s.size - 1
    j0 = row_index(vec_v, V_0)
    row = np.asarray(U, dtype=np.float64)[j0 * (m1 + 1):(j0 + 1) * (m1 + 1)]
    spots = np.asarray(spots, dtype=np.float64).reshape(-1)
    scales = np.ones_like(spots) if scales is None else np.asarray(scales, dtype=np.float64).reshape(-1)
    val, amp, flags = np.empty(spots.size), np.empty(spots.size), np.zeros(spots.size, dtype=np.int32)
    for q, (x, c) in enumerate(zip(spots, scales)):
        idx, w, flags[q] = taps(s, x)
        if flags[q]:
            val[q], amp[q] = np.nan, 0.0
            continue
        u = row[idx]
        val[q] = (((w[0] * u[0]) + w[1] * u[1]) + w[2] * u[2]) + w[3] * u[3]
        val[q] *= c
        amp[q] = np.abs(w).sum() * abs(c)
    return val, amp, flags


def sample_batch(U, vec_s, vec_v, V_0, spots, scales=None):
    """A batch: U [n][m], grids [n][..], V_0 a scalar or [n], spots / scales [n_samp] (one list) or [n][n_samp].
    Returns (values, sum|w| |scale|, flags), each [n][n_samp]."""
    n = np.asarray(U).shape[0]
    sp = np.atleast_2d(np.asarray(spots, dtype=np.float64))
    sc = None if scales is None else np.atleast_2d(np.asarray(scales, dtype=np.float64))
    v0 = np.broadcast_to(np.asarray(V_0, dtype=np.float64), (n,))
    out = [sample_field(U[k], vec_s[k], vec_v[k], v0[k], sp[k if sp.shape[0] > 1 else 0],
                        None if sc is None else sc[k if sc.shape[0] > 1 else 0]) for k in range(n)]
    return tuple(np.stack([o[c] for o in out]) for c in range(3))


def kernel_test_spots(vec_s, S_0):
    """The ten spots the kernel tests use, for one s-grid (every kind the definition distinguishes): S_0 itself, two other nodes, five interior off-node spots, one
    in the first interval and one in the last (the clamped stencils)."""
    s = np.asarray(vec_s, dtype=np.float64)
    m1 = s.size - 1
    mid = lambda i, f: s[i] + f * (s[i + 1] - s[i])
    inner = [max(2, m1 // 7), max(3, m1 // 3), m1 // 2, max(4, (2 * m1) // 3), m1 - 3]
    fr = [0.37, 0.5, 0.81, 0.13, 0.66]
    return np.array([S_0, s[min(7, m1 - 1)], s[m1 - 2]] + [mid(i, f) for i, f in zip(inner, fr)] + [mid(0, 0.4), mid(m1 - 1, 0.6)])
