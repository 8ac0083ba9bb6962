"""The admitted domain of the Bates sub-step as one table, and the rule that judges ONE sub-step in isolation.  Plain data and
numpy, shared by tests/test_jumps_exact.py (the generator against mpmath), tests/test_emu_jump_domain.py (wave emulator),
tests/test_gpu_jump_domain.py and tests/cpp/jump_substep_san.cpp (the shapes, restated there).

The isolation.  One sub-step is U = P + a (G P) row by row, P the field in front of it.  Given the matrix G_dev the kernel itself
multiplies with (hadi_debug_jump_matrix / hadi_jump_matrix_unpack_kernel) the reference R = a (P @ G_dev^T) is formed in
np.longdouble (unit round-off 5.4e-20, no BLAS: numpy has none for that type), and D = U - P is held to the bound of a
floating-point inner product of K terms followed by one multiplication and one addition (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 3.1),

    |D - R|[j, i] <= a gamma(K + 2) (|P| @ |G_dev|^T)[j, i] + 2 u max(|U|, |P|)[j, i],   gamma(n) = n u / (1 - n u),  u = 2^-53,

K the padded K extent of the product, 4 hadi_jump_kg.  The bound is derived, not measured, and holds for every summation order.
The field is ROUGH, rng.uniform(0.5, 1.5) (1 + s_i) per node, so that every (output block, K tile) pair of a dense G carries
weight: on the smooth option values of the sweep tests a dropped far tile moves the field by less than their 1e-10."""
import functools

import numpy as np

from oracle import oracle as O

import common as Cm

# (mu_J, sigma_J): the laws of the accuracy table.  On well-conditioned grids numpy's generator stays within the entry bound of
# every one of them against a 40-digit generator at every width of M1_EDGES (tests/test_jumps_exact.py; worst 0.24 of the bound).
# DROPPED from the eight that were verified at m1 = 50: (0, 0.01) and (0, 0.02).  Their kbar is 5e-5 and 2e-4, so their bound stays
# 1e-13 on every row while the formula's error grows like u s_i / h: against 40 digits the numpy generator itself is at 0.13 of the
# bound at m1 = 50 and 65, but at 1.34 (m1 = 129), 2.76 (513) and 7.5 (1024).  The bound is not widened for them.
LAWS = ((-0.1, 0.15), (-1.0, 0.5), (0.5, 1.0), (0.0, 2.0), (-3.0, 0.1), (1.0, 0.05))
# ... of which these fill the whole matrix (every entry above 1e-8 at (0.5, 1.0))
DENSE = ((0.5, 1.0), (-1.0, 0.5), (0.0, 2.0))
MILD = ((-0.10, 0.15), (0.10, 0.30), (-0.20, 0.25))
# hadi_pick_shape changes the layout at 64 | 65, 128 | 129, 256 | 257, 512 | 513; 1024 is the last admitted width, 2 the first;
# 15, 16, 17: one 16-slot output block and its neighbour; 63, 64, 127, ...: a layout nearly full and full
M1_EDGES = (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
M1_M2 = 12
# rows nrows = m2 + 1 against the 64-row pass of the product (HADI_JUMP_ROWS) and its 16-row wavefront tiles: 4 (the minimum), 15,
# 16, 17, 48, 49, 63, 64, 65, 128, 129 and 528 (the streaming maximum)
M2_EDGES = (3, 14, 15, 16, 47, 48, 62, 63, 64, 127, 128, 527)
M2_M1 = 50
DT = 1e-6
WEIGHTS = (1.0, 0.37)  # a = lambda dt; 1 is the admitted edge
U_ROUND = 2.0 ** -53
ENTRY_BOUND = 1e-13


def gamma(n):
    return n * U_ROUND / (1.0 - n * U_ROUND)


def pick_shape(m1):
    """hadi_pick_shape for the streaming widths."""
    assert 2 <= m1 <= 1024
    return (1, 1) if m1 <= 64 else (2, 1) if m1 <= 128 else (4, 1) if m1 <= 256 else (8, 1) if m1 <= 512 else (8, 2)


def k_extent(m1):
    """The padded K extent of the product, 4 hadi_jump_kg: the row pitch 64 B G + 8 rounded up to whole tiles of 32 slots."""
    B, G = pick_shape(m1)
    return (64 * B * G + 8 + 31) // 32 * 32


def slot_of(m1, i):
    """hadi_pos: the slot of node i in a packed row."""
    B, G = pick_shape(m1)
    if i == 0:
        return 64 * B * G
    e = i - 1
    g, el = divmod(e, 64 * B)
    if B == 1:
        return 64 * g + el
    lane, r = divmod(el, B)
    return (r >> 1) * 128 * G + 128 * g + 2 * lane + (r & 1)


def node_of(m1, slot):
    """The node at a slot (hadi_slot_to_i), or None: a pad slot or a slot of a node beyond m1."""
    for i in range(m1 + 1):
        if slot_of(m1, i) == slot:
            return i
    return None


STRIKES = (100.0, 92.5, 108.0, 97.0, 103.5, 88.0, 112.0, 95.0)


@functools.lru_cache(maxsize=None)
def s_grids(m1, n, same=False):
    """[n][m1 + 1] s-grids of the project's builder, one strike each (same: instance 0's for all).  The builder serves every
    m1 >= 2.  Nothing is asked of their conditioning: the isolation's bound needs none."""
    K = [STRIKES[0 if same else k % len(STRIKES)] * (1.0 + 0.001 * (0 if same else k // len(STRIKES))) for k in range(n)]
    G = [O.grid(m1, 8 * k, Cm.S_0, k, k / 5, 8, 5.0, Cm.V_0, 5.0 / 500) for k in K]
    vs, ds = (np.ascontiguousarray(np.stack([g[j] for g in G])) for j in (0, 2))
    assert (np.diff(vs, axis=1) > 0).all() and np.array_equal(ds, vs[:, 1:] - vs[:, :-1])
    vs.setflags(write=False)
    ds.setflags(write=False)
    return vs, ds


@functools.lru_cache(maxsize=None)
def v_grid(m2):
    vv, dv = O.rebuild_variance(m2, Cm.v0_for(m2))
    vv.setflags(write=False)
    dv.setflags(write=False)
    return vv, dv


def rough_field(seed, vs, m2):
    """[n][(m2 + 1)(m1 + 1)]: uniform(0.5, 1.5) (1 + s_i) per node, seeded."""
    rng = np.random.default_rng(seed)
    n, m1p = vs.shape
    F = rng.uniform(0.5, 1.5, size=(n, m2 + 1, m1p)) * (1.0 + vs[:, None, :])
    return np.ascontiguousarray(F.reshape(n, -1))


def roughness(F, m1, m2):
    """Median relative difference between s-neighbours of one field."""
    X = np.abs(F.reshape(m2 + 1, m1 + 1)[:, 1:])
    return float(np.median(np.abs(np.diff(X, axis=1)) / np.maximum(X[:, 1:], X[:, :-1])))


def laws_for(n, first=0, pool=DENSE + MILD):
    """(mu [n], sigma [n]): the dense laws first."""
    return (np.array([pool[(first + k) % len(pool)][0] for k in range(n)]), np.array([pool[(first + k) % len(pool)][1] for k in range(n)]))


def intensity(a, dt=DT):
    """The largest lambda with fl(lambda dt) <= a: the library forms the weight as that product and refuses one above 1."""
    lam = a / dt
    while lam * dt > a:
        lam = np.nextafter(lam, 0.0)
    return float(lam)


def stiffness(vs):
    """max_i s_i / min(h_{i-1}, h_i): what the explicit compensator a kbar s d/ds multiplies round-off by, per unit a |kbar|."""
    ds = np.diff(vs)
    return float((vs / np.minimum(np.r_[ds[0], ds], np.r_[ds, ds[-1]])).max())


def stable_intensity(vs, mu, sigma, dt, margin=0.9):
    """lambda with a |kbar| max(s_i / h_i) = margin <= 1 on the grid vs, a = lambda dt (and a <= 1)."""
    import jumps_ref as JR
    return min(1.0, margin / (abs(JR.kbar(mu, sigma)) * stiffness(vs))) / dt


def substep_ratio(P, U, G, a, m1, m2, perturb=None):
    """The worst |D - R| over its bound for ONE instance (a module docstring has the bound), and where.  P, U [(m2+1)(m1+1)]: the
    field in front of and behind the sub-step; G [m1+1][m1+1]: the device's own matrix; a: the weight as the device forms it.
    perturb (i, l, rel): G[i][l] moves by rel max|G[i]| on the REFERENCE side only -- the self-test of the rule's teeth.
    Column 0 (s = 0: row 0 of G is zero) must not move at all."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1.1e-19, "np.longdouble is not the x87 extended type here"
    Pm, Um = P.reshape(m2 + 1, m1 + 1), U.reshape(m2 + 1, m1 + 1)
    assert np.isfinite(Um).all() and np.array_equal(Um[:, 0], Pm[:, 0]), "column 0 moved"
    Gx = G.astype(LD)
    if perturb is not None:
        i, l, rel = perturb
        Gx[i, l] += LD(rel) * LD(np.abs(G[i]).max())
    # (object-free longdouble products: numpy falls back to its own loops for this type, no BLAS)
    R = LD(a) * (Pm.astype(LD) @ Gx.T)
    D = Um.astype(LD) - Pm.astype(LD)
    bound = LD(a) * LD(gamma(k_extent(m1) + 2)) * (np.abs(Pm).astype(LD) @ np.abs(G).astype(LD).T) + \
        LD(2.0 * U_ROUND) * np.maximum(np.abs(Um), np.abs(Pm)).astype(LD)
    err = np.abs(D - R)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    j, i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[j, i]), (int(j), int(i))


def teeth_positions(m1):
    """(output node, input node) of the self-test: a near pair, a far pair (first output block against the last nodes' K tile) and
    one whose input slot lies in the LAST K tile that holds a node."""
    last_tile = max(range(m1 + 1), key=lambda i: slot_of(m1, i) // 32)
    return {"near": (min(2, m1), 1), "far": (1, m1), "last K tile": (max(1, m1 // 2), last_tile)}


def entry_bound(vs, mu, sigma):
    """[m1 + 1]: the suite's bound on an entry of row i, 1e-13 max(1, |kbar| s_i / min(h_{i-1}, h_i))."""
    import jumps_ref as JR
    ds = np.diff(vs)
    hmin = np.minimum(np.r_[ds[0], ds], np.r_[ds, ds[-1]])
    return ENTRY_BOUND * np.maximum(1.0, abs(JR.kbar(mu, sigma)) * vs / hmin)


# ---- ill-conditioned s-grids: the placements of tests/ill_grids.py with one interval 1e6 times shorter than its neighbour ---------
ILL_R = 1e6
ILL_SHAPES = ((50, 12), (600, 8))
ILL_LAWS = ((-0.1, 0.15), (0.5, 1.0), (-1.0, 0.5))
ILL_FIXTURE = "jump_exact_ill.json"


@functools.lru_cache(maxsize=None)
def ill_s_grids(m1):
    """((name, Vec_s, Delta_s, t), ...): every placement of ill_grids.s_positions(m1, K), sides alternating; the tiny interval is
    [s_t, s_t+1]."""
    import ill_grids as IG
    K = Cm.well_conditioned_strikes(m1, 1)[0]
    out = []
    for p, (name, kind, t) in enumerate(IG.s_positions(m1, K)):
        side = IG.SIDES[p % 2]
        si = IG._raw_index(kind, t, side)
        raw = IG.raw_s(m1, K)
        vs, ds, _ = IG.s_grid(m1, K, si, IG.fit_ratio(raw[si + 1] - raw[si], ILL_R), side)
        tiny = int(np.argmin(ds))
        assert Cm.interval_ratios(ds)[0] >= 1e5 and 0 <= tiny < m1
        vs.setflags(write=False)
        ds.setflags(write=False)
        out.append((name, vs, ds, tiny))
    return tuple(out), K


def ill_rows(m1, tiny):
    """matrix_rows and the two nodes of the tiny interval."""
    return sorted(set(matrix_rows(m1)) | {max(1, tiny), tiny + 1})


def ill_key(m1, name, law):
    return "%d|%s|%g|%g" % (m1, name, law[0], law[1])


FACTOR = 30.0  # ill_grids.FACTOR
LD = np.longdouble


# The round-off of the STORED entries: an entry of G is the result of at most 20 rounded operations (hadi_jump_piece: two quotients,
# two logarithms, four erfc and their differences, the two products and the sum; hadi_jump_entry_value: the interval, the stencil
# weight, kbar s_i times it, the sums), so it sits within gamma(20) of the magnitudes it is made of.  On well-conditioned grids the
# term is below 1e-13; beside an interval of 1e-6 the compensator's entries are kbar s_i / h = 2e7, and no fp64 matrix has |G s|
# below 2e7 u s = 4e-7 there.
ENTRY_OPS = 20


def row_sums_ratio(G, vs, ops=0):
    """max(|G 1|, |G s|) over 1e-12 max s (+ gamma(ops) |G| |x|), the sums in np.longdouble so that the check adds no round-off of
    its own (a BLAS product of a 1025-wide row of entries of 30 adds 2e-9)."""
    A, worst = np.abs(G).astype(LD), 0.0
    for x in (np.ones(vs.size), vs):
        got = np.abs(G.astype(LD) @ x.astype(LD))
        worst = max(worst, float((got / (LD(1e-12 * vs.max()) + LD(gamma(ops)) * (A @ np.abs(x).astype(LD)))).max()))
    return worst


def term_magnitudes(vs, mu, sigma):
    """T [m1+1][m1+1]: the magnitudes an entry of G is made of -- jumps_ref.expectation_matrix with every product taken in absolute
    value and every difference Phi(d1) - Phi(d0) replaced by the sum of the two tail values it is formed from, plus the identity and
    |kbar| s_i |D|.  gamma(ENTRY_OPS) T[i][l] is the a-priori round-off of entry (i, l) in ANY fp64 evaluation of the formula: it is
    below 1e-13 everywhere on a well-conditioned grid and reaches 1e-8 in the two columns around an interval of 1e-6, where
    a = s / h = 3e7 multiplies tail values of 1e-2."""
    import jumps_ref as JR
    from scipy.special import ndtr
    vs = np.asarray(vs, dtype=np.float64)
    m1 = vs.size - 1
    kb = JR.kbar(mu, sigma)
    T = np.zeros((m1 + 1, m1 + 1))
    si = vs[1:]

    def d(x):
        if x <= 0.0 or np.isinf(x):
            return np.full(si.shape, -np.inf if x <= 0.0 else np.inf)
        return (np.log(x / si) - mu) / sigma

    def tails(d0, d1):
        return np.where(d0 > 0.0, ndtr(-d0) + ndtr(-d1), ndtr(d1) + ndtr(d0))

    for q in range(m1):
        x0, x1 = vs[q], (vs[q + 1] if q < m1 - 1 else np.inf)
        h = vs[q + 1] - vs[q]
        d0, d1 = d(x0), d(x1)
        M0, M1 = tails(d0, d1), tails(d0 - sigma, d1 - sigma)
        w = (1.0 / h) * si * (1.0 + kb) * M1
        T[1:, q] += (vs[q + 1] / h) * M0 + w
        T[1:, q + 1] += (vs[q] / h) * M0 + w
    T += np.eye(m1 + 1) + abs(kb) * vs[:, None] * np.abs(JR.derivative_matrix(vs))
    T[0, :] = 0.0
    return T


def _generator(vs, mu, sigma):
    import jumps_ref as JR
    return JR.generator(vs, mu, sigma)


def ill_matrix_check(name, G, vs, K, tiny, law, rec):
    """The device matrix on an ill grid against the numpy generator: entries at max(entry bound, 30 x the numpy formula's recorded
    distance from 40 digits on that row, the entry's own a-priori round-off gamma(ENTRY_OPS) T[i][l]) -- the recorded distance is ONE
    realisation of that round-off (measured: 7.5e-15 on a row whose entries are 6e5, half an ulp of which is 7e-11), so without the
    third term an independent evaluation fails by the luck of the reference's draw --, the two-column sum likewise, the action on the two payoffs at 1e-13 of max |G||u|, the row sums
    at 1e-12 max s -- the last three with the round-off of the stored entries (tests/test_jumps_exact.py).  Returns the margins."""
    m1 = vs.size - 1
    rows = rec["rows"]
    Gr = _generator(vs, *law)
    b = entry_bound(vs, *law)[rows]
    assert np.isfinite(G).all() and not G[0].any()
    T = gamma(ENTRY_OPS) * term_magnitudes(vs, *law)[rows]
    r_entry = (np.abs(G[rows] - Gr[rows]) / np.maximum(np.maximum(b, FACTOR * np.array(rec["dist"]))[:, None], T)).max()
    sd = np.abs((G[rows, tiny].astype(LD) + G[rows, tiny + 1].astype(LD)) - (Gr[rows, tiny].astype(LD) + Gr[rows, tiny + 1].astype(LD))).astype(np.float64)
    rep = gamma(ENTRY_OPS) * (np.abs(Gr[rows, tiny]) + np.abs(Gr[rows, tiny + 1]))
    r_sum = (sd / (np.maximum(b, FACTOR * np.array(rec["sum_dist"])) + 2 * rep)).max()
    A = np.abs(G).astype(LD)
    r_rs = row_sums_ratio(G, vs, ENTRY_OPS)
    r_act = 0.0
    for u in (np.maximum(vs - K, 0.0), np.maximum(K - vs, 0.0)):
        d = np.abs(G.astype(LD) @ u.astype(LD) - Gr.astype(LD) @ u.astype(LD)).astype(np.float64)
        sc = (A @ np.abs(u).astype(LD)).astype(np.float64)
        r_act = max(r_act, d.max() / (1e-13 * sc.max()))
    print("%s (%g, %g): entries %.3f, two-column sum %.3f, action %.3f, row sums %.3f of their bounds" % (name, law[0], law[1], r_entry, r_sum, r_act, r_rs))
    return r_entry, r_sum, r_act, r_rs


def matrix_rows(m1):
    """The rows of G that the 40-digit generator checks: all of them up to m1 = 129; above, a fixed set of at most 32 -- i = 1, 2,
    m1 - 1, m1, the nodes at slots 0, 15, 16 of a 16-slot block (the first, one in the middle, the last that holds nodes), i = 512,
    513 where two wavefronts share a row, and an even spread."""
    if m1 <= 129:
        return list(range(1, m1 + 1))
    rows = {1, 2, m1 - 1, m1}
    nodes = {slot_of(m1, i): i for i in range(m1 + 1)}
    blocks = sorted({s // 16 for s in nodes})
    for b in (blocks[0], blocks[len(blocks) // 2], blocks[-2]):
        rows.update(nodes[16 * b + k] for k in (0, 15) if 16 * b + k in nodes)
        if 16 * (b + 1) in nodes:
            rows.add(nodes[16 * (b + 1)])
    if m1 > 512:
        rows.update((512, 513))
    rows.discard(0)
    spread = [int(x) for x in np.linspace(3, m1 - 2, 32)]
    for i in spread:
        if len(rows) >= 32:
            break
        rows.add(i)
    assert len(rows) <= 32
    return sorted(rows)
