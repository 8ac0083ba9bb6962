"""Spots, sample counts and the tight check shared by the sample-domain tests of the sampled ladder
(tests/test_emu_sample_domain.py on the CPU, tests/test_gpu_sample_domain.py on the device).  Plain data and numpy helpers; the
grids are event_cases' (SHAPES, LDS_ROWS, oracle_batch: asserted well-conditioned).

domain_spots(vec_s, S_0, budget) lists, for ONE s-grid, in this order
  column 0      S_0 (a node of every grid here): the column that equals the ladder bit for bit
  node hits     scale 1.0: s_0, s_m1, s_1 and every node of the reference stencil (samples_ref.taps) of every interior spot of the
                list -- so the call itself returns the bits of every state element its interior samples read
  interior      one spot in each chosen interval, fractions cycling over FRACTIONS, scales over SCALES.  The intervals, by rank:
                0, 1, 2, m1-3, m1-2, m1-1 (either side of where the clamp i0 = min(max(i - 1, 0), m1 - 3) stops acting); the two
                intervals at S_0; the intervals within two of the wave edge 1 + 64 B (G = 2), of every 64-slot group edge (above
                1024 nodes) and of the lane edges 1 + B l (B > 1); then every other interval.  Lane edges and the rest are taken in
                an evenly spreading order (bit reversal), and an interval is taken while it and the stencil nodes it adds still fit
                the budget: every interval with all three fractions when 4 m1 + 16 <= budget, an even sample of the lanes above that
                (1024 is the library's maximum, and B = 8 rows have more lane edges than that).
  tolerance     on a node s_t with 1 <= s_t <= 200: s_t -+ 5e-11 (hits), s_t -+ 2e-10 (interior, the stencil of the interval they
                fall in), 0.0 and -5e-11 (hits of node 0: s_0 = 1.42e-14 on every grid here, so both lie BELOW the grid),
                s_m1 + 5e-11 (above the grid, a hit)
Every entry is asserted, with samples_ref alone, to have the kind it is named for and flag 0, and every interior one sum|w| <= 16
(measured maximum over SHAPES and LDS_ROWS: 11.361 at 256x8) -- conditions on the inputs, never filters.

The tight check.  For an interior sample the reference is samples_ref's chain applied to the NODE-HIT COLUMNS OF THE SAME CALL AND
SNAPSHOT (scale 1, so they are the state's bits), and |out - ref| <= 32 * 2^-53 * sum_a |w_a u_a| * |scale|: four products and
three sums round once each in the reference, one product and three FMAs on the device, the scale once on each side -- under 12
units; the rest is margin for a last-bit difference in a weight (seven roundings each).  Derived, not measured.  A tolerance hit
(scale != 1) is the node's column times the scale, bit for bit."""
import numpy as np

import samples_ref as R
from event_cases import LDS_ROWS, SHAPES, oracle_batch, pick_shape  # noqa: F401  (re-exported: the tests' one table)

COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 1024)
COUNTS_WHAT = {1: "S_0 alone", 31: "below the pairs kernel's stride", 32: "the pairs kernel's stride exactly", 33: "one lane of a half loops twice",
               63: "below one wavefront", 64: "seq / sch stride exactly", 65: "one lane of seq / sch loops twice", 255: "below one block of 256",
               256: "block4's stride and one block exactly", 257: "one thread of block4 loops twice; a second block of one thread",
               511: "below block8's stride", 513: "one thread of block8 loops twice", 1024: "the documented maximum"}
FRACTIONS = (0.13, 0.5, 0.87)
SCALES = (0.75, -1.25, 3.0, 0.3)
AMP_MAX = 16.0
TIGHT = 32 * 2.0 ** -53
S0, HIT, INTERIOR, TOL_HIT, TOL_INTERIOR = range(5)


def _bitrev_order(n):
    """0 .. n-1 in an order whose every prefix is spread evenly."""
    bits = max(1, (n - 1).bit_length())
    return [r for r in (int(format(k, "0%db" % bits)[::-1], 2) for k in range(1 << bits)) if r < n]


def ranked_intervals(m1, i_s0):
    """Every interval 0 .. m1-1 once, in the rank of the module's docstring."""
    B, G = pick_shape(m1)
    around = lambda e: [i for i in (e - 2, e - 1, e, e + 1) if 0 <= i < m1]
    out = [i for i in (0, 1, 2, m1 - 3, m1 - 2, m1 - 1) if 0 <= i < m1] + [i for i in (i_s0 - 1, i_s0) if 0 <= i < m1]
    if G == 2:
        out += around(1 + 64 * B)
    if m1 > 1024:
        for g in range(1, G):
            out += around(1 + 64 * g)
    if B > 1:
        lanes = [l for l in range(64 * G) if 1 + B * l <= m1]
        for k in _bitrev_order(len(lanes)):
            out += around(1 + B * lanes[k])
    out += _bitrev_order(m1)
    seen, uniq = set(), []
    for i in out:
        if i not in seen:
            seen.add(i)
            uniq.append(i)
    assert sorted(uniq) == list(range(m1))
    return uniq


def _pad_fraction(j):
    return 0.05 + 0.9 * ((0.6180339887498949 * (j + 1)) % 1.0)


def domain_spots(vec_s, S_0, budget=1024, length=None):
    """(spots, scales, kinds) of one s-grid; length: cut to, or padded up to, that many entries by further interior spots (other
    fractions of intervals already chosen, so their stencil nodes are hits of the list)."""
    s = np.asarray(vec_s, dtype=np.float64)
    m1 = s.size - 1
    assert m1 >= 8 and budget >= 64
    i_s0 = int(np.nonzero(s == S_0)[0][0])
    mid = lambda i, f: s[i] + f * (s[i + 1] - s[i])
    stencil = lambda i: range(min(max(i - 1, 0), m1 - 3), min(max(i - 1, 0), m1 - 3) + 4)
    # the tolerance block: the middle node among those with 1 <= s_t <= 200 (away from the clamped ends)
    cand = [i for i in range(3, m1 - 2) if 1.0 <= s[i] <= 200.0]
    t = cand[len(cand) // 2]
    tol = [(s[t] - 5e-11, TOL_HIT), (s[t] + 5e-11, TOL_HIT), (s[t] - 2e-10, TOL_INTERIOR), (s[t] + 2e-10, TOL_INTERIOR),
           (0.0, TOL_HIT), (-5e-11, TOL_HIT), (s[m1] + 5e-11, TOL_HIT)]
    hits = [0, m1, 1]
    for i in (t - 1, t):  # (the two stencils of s_t -+ 2e-10)
        hits += [a for a in stencil(i) if a not in hits]
    room = budget - 1 - len(tol)
    chosen = []  # (interval, fraction)
    ranked = ranked_intervals(m1, i_s0)
    first = set()
    for f_turn in range(3):
        for k, i in enumerate(ranked):
            if f_turn and i not in first:
                continue  # (further fractions only where the first one fitted: their nodes are hits already)
            new = [a for a in stencil(i) if a not in hits]
            if len(hits) + len(new) + len(chosen) + 1 <= room:
                hits += new
                first.add(i)
                chosen.append((i, FRACTIONS[(k + f_turn) % 3]))
    spots = [S_0] + [s[i] for i in hits] + [mid(i, f) for i, f in chosen] + [x for x, _ in tol]
    kinds = [S0] + [HIT] * len(hits) + [INTERIOR] * len(chosen) + [k for _, k in tol]
    if length is not None:
        j = 0
        while len(spots) < length:
            i = chosen[j % len(chosen)][0]
            spots.append(mid(i, _pad_fraction(j)))
            kinds.append(INTERIOR)
            j += 1
        spots, kinds = spots[:length], kinds[:length]
    assert len(spots) <= budget or length is not None
    spots, kinds = np.array(spots), np.array(kinds)
    scales = np.ones(spots.size)
    other = np.nonzero((kinds != S0) & (kinds != HIT))[0]
    scales[other] = [SCALES[k % len(SCALES)] for k in range(other.size)]
    _assert_kinds(s, spots, kinds)
    return spots, scales, kinds


_TAPS = {}


def _taps(skey, s, x):
    """samples_ref.taps, kept per (grid, spot): the count cases are prefixes of one list."""
    key = (skey, float(x))
    if key not in _TAPS:
        _TAPS[key] = R.taps(s, x)
    return _TAPS[key]


def _assert_kinds(s, spots, kinds):
    """With samples_ref alone: every entry has the kind it is named for and flag 0; interior ones have sum|w| <= AMP_MAX."""
    m1 = s.size - 1
    skey = s.tobytes()
    for x, k in zip(spots, kinds):
        idx, w, flag = _taps(skey, s, x)
        assert flag == 0, (x, k)
        hit = idx[0] == idx[3]
        assert hit == (k in (S0, HIT, TOL_HIT)), (x, k, idx)
        if not hit:
            assert np.abs(w).sum() <= AMP_MAX, (x, np.abs(w).sum())  # choose another fraction for that interval if this ever fails
            assert s[idx[0]] < x < s[idx[3]] and idx[0] == min(max(int(np.nonzero(s < x)[0][-1]) - 1, 0), m1 - 3)


_CACHE = {}


def batch_spots(vec_s, S_0, budget=1024, count=None):
    """(spots, scales, kinds), each [n][n_samp]: domain_spots of every instance's own grid, rows padded to the longest (count:
    every row cut or padded to exactly count entries).  Built once per input and left unchanged."""
    vs = np.asarray(vec_s)
    key = (vs.tobytes(), S_0, budget, count)
    if key not in _CACHE:
        n = vs.shape[0]
        L = count if count is not None else max(domain_spots(vs[k], S_0, budget)[0].size for k in range(n))
        assert L <= max(budget, count or 0)
        rows = [domain_spots(vs[k], S_0, budget, length=L) for k in range(n)]
        out = tuple(np.ascontiguousarray(np.stack([r[c] for r in rows])) for c in range(3))
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


_STENCILS = {}


def stencils(vec_s, spots):
    """samples_ref.taps of every sample of a batch: (idx [n][n_samp][4], w [n][n_samp][4]); flags asserted 0.  Kept per input."""
    vs, sp = np.asarray(vec_s), np.asarray(spots)
    key = (vs.tobytes(), sp.tobytes())
    if key not in _STENCILS:
        n, ns = sp.shape
        idx, w = np.empty((n, ns, 4), dtype=np.int64), np.empty((n, ns, 4))
        for k in range(n):
            s = np.asarray(vs[k], dtype=np.float64)
            skey = s.tobytes()
            for q in range(ns):
                idx[k, q], w[k, q], flag = _taps(skey, s, sp[k, q])
                assert flag == 0
        _STENCILS[key] = (idx, w)
    return _STENCILS[key]


def tight_check(out, vec_s, spots, scales, name=""):
    """out [n][n_snap][n_samp] of ONE call.  Asserts the tight bound on every interior sample and bit equality on every hit with a
    scale; returns (worst |diff| / bound, interior samples checked).  Every stencil node must be a scale-1 hit of the same row."""
    out, scales = np.asarray(out), np.asarray(scales)
    idx, w = stencils(vec_s, spots)
    worst, count = 0.0, 0
    for k in range(out.shape[0]):
        is_hit = idx[k, :, 0] == idx[k, :, 3]
        col = {}
        for q in np.nonzero(is_hit & (scales[k] == 1.0))[0]:
            col.setdefault(int(idx[k, q, 0]), int(q))
        for q in np.nonzero(is_hit & (scales[k] != 1.0))[0]:
            assert np.array_equal(out[k, :, q], out[k, :, col[int(idx[k, q, 0])]] * scales[k, q]), (name, k, q)
        rows = np.nonzero(~is_hit)[0]
        if not rows.size:
            continue
        cols = np.array([[col[int(a)] for a in idx[k, q]] for q in rows])  # (KeyError: a stencil node that is no hit of the list)
        u = out[k][:, cols]                                                # [n_snap][rows][4]
        wk, c = w[k, rows], scales[k, rows]
        ref = ((((wk[:, 0] * u[..., 0]) + wk[:, 1] * u[..., 1]) + wk[:, 2] * u[..., 2]) + wk[:, 3] * u[..., 3]) * c
        bound = TIGHT * np.abs(wk * u).sum(axis=-1) * np.abs(c)
        diff = np.abs(out[k][:, rows] - ref)
        assert np.isfinite(out[k]).all(), (name, k)
        bad = diff > bound
        assert not bad.any(), (name, k, [(int(rows[b[1]]), float(diff[tuple(b)] / bound[tuple(b)])) for b in np.argwhere(bad)[:4]])
        worst = max(worst, float((diff[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
        count += rows.size
    return worst, count


def synthetic_field(m1, m2, n):
    """U[k][i + j (m1 + 1)] = (i + 1) + 4096 (j + 1) + 2^23 k: a wrong node, row or instance moves a sample by at least 1."""
    i, j = np.arange(m1 + 1), np.arange(m2 + 1)
    one = ((i + 1)[None, :] + 4096.0 * (j + 1)[:, None]).reshape(-1)
    return np.ascontiguousarray(np.stack([one + 2.0 ** 23 * k for k in range(n)]))


# ---- locate edges on synthetic increasing grids ---------------------------------------------------------------------------------
# (name, s-grid, [(spot, expectation)]), the expectations written out BY HAND from the definition in include/hadi.h:
# ("hit", i): node i's value; ("interior", i0): the stencil i0 .. i0 + 3, flag 0; ("off",): NaN, OFF_GRID; ("deg",): NaN, DEGENERATE.
# tests/test_samples_ref.py pins samples_ref to this table, tests/test_emu_sample_domain.py the locate kernel.
_INF, _NAN = float("inf"), float("nan")
LOCATE_EDGES = [
    ("m1 = 2: hits are fine, every interior spot is degenerate", [1.0, 2.0, 4.0],
     [(1.0, ("hit", 0)), (2.0, ("hit", 1)), (4.0, ("hit", 2)), (2.0 + 5e-11, ("hit", 1)), (1.5, ("deg",)), (3.0, ("deg",)), (4.5, ("off",))]),
    ("m1 = 3: one stencil for every interior spot", [1.0, 2.0, 4.0, 8.0],
     [(1.5, ("interior", 0)), (3.0, ("interior", 0)), (5.0, ("interior", 0)), (7.999, ("interior", 0)), (8.0, ("hit", 3)), (1.0, ("hit", 0))]),
    ("two nodes 5e-11 apart: the first wins; a stencil holding both is not degenerate", [1.0, 2.0, 2.0 + 5e-11, 3.0, 4.0, 5.0],
     [(2.0 + 5e-11, ("hit", 1)), (2.0 + 2.5e-11, ("hit", 1)), (2.0 + 1.2e-10, ("hit", 2)), (2.0 - 5e-11, ("hit", 1)), (2.6, ("interior", 1)),
      (1.5, ("interior", 0)), (3.5, ("interior", 2)), (4.5, ("interior", 2))]),
    ("an equal pair: degenerate inside the stencil, flag 0 outside it", [1.0, 2.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0],
     [(2.0, ("hit", 1)), (2.5, ("deg",)), (1.5, ("deg",)), (3.5, ("interior", 2)), (5.5, ("interior", 4)), (6.5, ("interior", 5)),
      (7.5, ("interior", 5)), (4.5, ("interior", 3))]),
    ("non-finite spots, signed zeros and the tolerance at both ends", [1e-14, 1.0, 2.0, 3.0, 5.0],
     [(_INF, ("off",)), (-_INF, ("off",)), (_NAN, ("off",)), (-0.0, ("hit", 0)), (0.0, ("hit", 0)), (-5e-11, ("hit", 0)), (-2e-10, ("off",)),
      (5.0 + 5e-11, ("hit", 4)), (5.0 + 2e-10, ("off",)), (2.5, ("interior", 1)), (0.5, ("interior", 0)), (1.0 + 2e-10, ("interior", 0)),
      (2.0 - 2e-10, ("interior", 0)), (2.0 + 2e-10, ("interior", 1))]),
]
