"""Reference-node placements, batches and schedules shared by the domain tests of the strike fixing (tests/test_emu_fixing_domain.py
on the CPU, tests/test_gpu_fixing_domain.py on the device).  Plain data and numpy helpers; the shapes, the batches and the schedules
next to dividends are those of tests/event_cases.py.

hadi_fixing_kernel visits the packed state in 16-byte PAIRS of slots (hadi_core.h, hadi_pos / hadi_slot_to_i): a pair whose two
slots are nodes takes one store, a pair with one node takes a single store of that half.  reference_nodes puts i_ref on every special
slot of a shape's (B, G): node 0 (slot 64 B G, whose partner is a pad), the last node (with an odd m1 the only node of its pair), the
ends of a lane, the two halves of an interior pair, the nodes on either side of the second wavefront, and on natural rows the nodes
around the 64-slot groups.  fixing_batch hands them out over a batch, `turn` walks the list over the runs of one (B, G) class.
"""
import numpy as np

import cliquet_ref as QR
import common as Cm
import event_cases as E

SHARES, RETURN = QR.SHARES, QR.RETURN
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)


# ---- the packed row: numpy copies of hadi_pos and hadi_slot_to_i -----------------------------------------------------------------
def pos(B, G, i):
    """Slot of node i (hadi_pos)."""
    if i == 0:
        return 64 * B * G
    e = i - 1
    g, el = divmod(e, 64 * B)
    if B == 1:
        return 64 * g + el
    lane, r = divmod(el, B)
    return (r >> 1) * 128 * G + 128 * g + 2 * lane + (r & 1)


def slot_to_i(B, G, slot):
    """Node stored in `slot`, -1 for a pad slot (hadi_slot_to_i); the result may lie beyond m1."""
    n = 64 * B * G
    if slot == n:
        return 0
    if slot > n:
        return -1
    if B == 1:
        return slot + 1
    q, rem = divmod(slot, 128 * G)
    g, rem2 = rem >> 7, rem & 127
    return 1 + 64 * B * g + B * (rem2 >> 1) + 2 * q + (rem2 & 1)


def pair_partner(m1, i):
    """What shares node i's 16-byte pair: a node index, or None where the other half is a pad slot or the slot of a node beyond m1."""
    B, G = E.pick_shape(m1)
    other = slot_to_i(B, G, pos(B, G, i) ^ 1)
    return other if 0 <= other <= m1 else None


# ---- placements -------------------------------------------------------------------------------------------------------------------
def reference_nodes(m1):
    """[(name, i_ref, mode)] for the (B, G) of m1 s-intervals."""
    B, G = E.pick_shape(m1)
    assert all(slot_to_i(B, G, pos(B, G, i)) == i for i in range(m1 + 1))
    odd = (m1 // 2) | 1
    assert 2 < odd and odd + 1 < m1 - 1 and pair_partner(m1, odd) == odd + 1 and pair_partner(m1, odd + 1) == odd
    out = [("node 0", 0, RETURN),  # (SHARES there is refused: s_0 is the grid's 0)
           ("node 1", 1, SHARES), ("node m1", m1, RETURN), ("node m1 - 1", m1 - 1, SHARES),
           ("last node of lane 0", B, RETURN), ("first node of lane 1", B + 1, SHARES),
           ("odd half of a pair, RETURN", odd, RETURN), ("even half of a pair, SHARES", odd + 1, SHARES),
           ("odd half of a pair, SHARES", odd, SHARES), ("even half of a pair, RETURN", odd + 1, RETURN)]
    if G == 2:
        out += [("last node of wavefront 0", 64 * B, SHARES), ("first node of wavefront 1", 64 * B + 1, RETURN)]
    if m1 > 1024:  # natural rows: node i >= 1 in slot i - 1, 64-slot groups
        out += [("natural node 64", 64, RETURN), ("natural node 65", 65, SHARES), ("natural node 1024", 1024, RETURN),
                ("natural node m1, SHARES", m1, SHARES)]
    assert pair_partner(m1, 0) is None  # node 0's partner is a pad
    if m1 % 2:
        assert pair_partner(m1, m1) is None  # the last node of an even number of nodes is the only node of its pair
    assert all(0 <= i <= m1 and (i > 0 or mode == RETURN) for _, i, mode in out)
    return out


def n_reference_nodes(m1):
    B, G = E.pick_shape(m1)
    return 10 + 2 * (G == 2) + 4 * (m1 > 1024)


def fixing_batch(vec_s, turn=0):
    """(ref_spot, mode, i_ref, names): instance k takes placement (k + turn) of reference_nodes; the spot is the instance's own
    node, and i_ref is what hadi_fixing_locate_kernel must find there (cliquet_ref.find_node: the price pick's rule)."""
    vs = np.asarray(vec_s, dtype=np.float64)
    n, m1 = vs.shape[0], vs.shape[1] - 1
    pl = reference_nodes(m1)
    ref, mode, i_ref, names = np.empty(n), [], [], []
    for k in range(n):
        name, i, md = pl[(k + turn) % len(pl)]
        ref[k] = vs[k][i]
        assert QR.find_node(vs[k], ref[k]) == i, (name, i)
        mode.append(md)
        i_ref.append(i)
        names.append(name)
    return ref, mode, i_ref, names


# ---- the streaming runs and their turns -------------------------------------------------------------------------------------------
TURN_STEP = 3  # the fewest instances a run has (the large shapes on the device)


def streaming_runs():
    """[(id, row of SHAPES, shape, strip tuning, turn)]: the ring and the strips of every class that has strips, the plan's own
    kernels below 65 and above 1024 s-intervals -- the rows and ids of the event-domain tests.  The runs of one (B, G) class take
    the turns 0, 3, 6, ..., so that already the first three instances of every run walk the class's placements; a class with too few
    runs for that (the natural rows: one shape) repeats its last row with further turns (ids ending in -turnK)."""
    out, per_class = [], {}
    for k, s in enumerate(E.SHAPES):
        for strip in ((0, 1) if 64 < s.m1 <= 1024 else (None,)):
            runs = per_class.setdefault(E.pick_shape(s.m1), [])
            sid = "%s-%dx%d-%s" % (s.name, s.m1, s.m2, {None: "plan", 0: "ring", 1: "strips"}[strip])
            runs.append(len(out))
            out.append((sid, k, s, strip, TURN_STEP * (len(runs) - 1)))
    for cls, runs in per_class.items():
        sid, k, s, strip, _ = out[runs[-1]]
        while TURN_STEP * len(runs) < n_reference_nodes(s.m1):
            runs.append(len(out))
            out.append(("%s-turn%d" % (sid, len(runs) - 1), k, s, strip, TURN_STEP * (len(runs) - 1)))
    return out


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def mixed_weights(fix, shift=0):
    """Zero and non-zero weights mixed, parallel to a schedule (one list or one list per instance); shift: where in the cycle the
    first instance starts."""
    cyc = (0.0, 1.0, 0.5, 0.0, 0.25)
    if fix and np.ndim(fix[0]) == 1:
        return [[cyc[(k + q + shift) % 5] for q in range(len(r))] for k, r in enumerate(fix)]
    return [cyc[(q + 1 + shift) % 5] for q in range(len(fix))]


def shape_schedule(n, N):
    """(fix_steps, weights) of the shape runs: every instance fixes at [1, N], each with its own row of weights -- at N the weights
    are 0, 1, 0.5, 0, 0.25 down the batch (at step 1: 0.25, 0, 1, 0.5, 0), so from three instances on both the bits-kept path
    (w == 0) and the + w P path run at N.  Instance 0 has weight 0 there, and in the first run of every (B, G) class it fixes at
    node 0; instances 0 and 3 stand three placements apart, which the tests use to meet a RETURN placement with weight 0 on
    every row with an odd m1."""
    fix = [[1, N] for _ in range(n)]
    w = mixed_weights(fix, 4)
    assert n < 3 or (any(r[-1] == 0.0 for r in w) and any(r[-1] != 0.0 for r in w))
    return fix, w


# ---- reference nodes around the strikes -------------------------------------------------------------------------------------------
# offsets from the node nearest the instance's strike, and modes, cycled through the batch (those of tests/test_gpu_cliquet.py)
NEAR_SHIFT, NEAR_MODES = (0, 3, -2, 1, -5), (SHARES, RETURN, RETURN, SHARES, RETURN)


def strike_batch(vec_s, strikes):
    """(ref_spot, mode, i_ref) with every instance's reference node a few nodes off its own strike."""
    vs = np.asarray(vec_s, dtype=np.float64)
    n = vs.shape[0]
    i_ref = [int(np.argmin(np.abs(vs[k] - strikes[k]))) + NEAR_SHIFT[k % 5] for k in range(n)]
    ref = np.array([vs[k][i_ref[k]] for k in range(n)])
    assert all(QR.find_node(vs[k], ref[k]) == i_ref[k] and 1 < i_ref[k] < vs.shape[1] - 1 for k in range(n))
    return ref, [NEAR_MODES[k % 5] for k in range(n)], i_ref


# ---- fixings next to dividends ----------------------------------------------------------------------------------------------------
def near_fixings(case, vec_s, strikes):
    """(fix_steps, weights, ref_spot, mode, i_ref) of three instances for a case of event_cases.schedules_near_dividends: the
    events are the fixing steps, with the mixed weights.  The reference nodes sit around the strikes -- except in the cases made
    for the jump's non-interpolating branches (barrier == "floor": big_cash, negative, zero), where the jump right after a fixing
    reads node 0 and the low nodes: there instance 0 is RETURN at node 0 (the whole row becomes node 0's value), instance 1 SHARES
    at node 1 (node 0 becomes exactly 0 times c: s_0 / s_1), instance 2 fixes near its strike."""
    vs = np.asarray(vec_s, dtype=np.float64)
    assert vs.shape[0] == 3
    _, mode, i_ref = strike_batch(vs, strikes)
    if case.barrier == "floor":
        i_ref, mode = [0, 1, i_ref[2]], [RETURN, SHARES, mode[2]]
    ref = np.array([vs[k][i_ref[k]] for k in range(3)])
    assert all(QR.find_node(vs[k], ref[k]) == i_ref[k] for k in range(3))
    fix = list(case.events)
    return fix, mixed_weights(fix), ref, mode, i_ref


# ---- rate and time regimes ----------------------------------------------------------------------------------------------------------
REGIMES = ["R0", "R6", "T3", "T5"]
REGIME_SHAPES = [(50, 25), (300, 80)]  # the ring and the sequential LDS kernel; the strips


def regime_inputs(rid, N0=3):
    """(rates, theta, dt, N, fix_steps, canon) of a regime of tests/regimes.py or tests/time_regimes.py for a row of N0 steps; canon:
    the rates, theta and dt of the canonical twin with the same N and the same fixings."""
    import regimes as R
    import time_regimes as TR
    if rid in R.RATE:
        rates, (theta, dt, N) = R.RATE[rid], TR.canonical(N0)
        canon = dict(rates=R.CANONICAL_RATES, theta=theta, dt=dt)
    else:
        rates, (theta, dt, N) = R.CANONICAL_RATES, TR.regime(rid, N0)
        canon = dict(rates=rates, theta=TR.canonical(N)[0], dt=TR.canonical(N)[1])
    return tuple(rates), theta, dt, N, ([1] if N == 1 else [1, N]), canon


# ---- the reference, once per distinct input ---------------------------------------------------------------------------------------
def freeze(x):
    if x is None or isinstance(x, (int, float, str, bool)):
        return x
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return tuple(freeze(y) for y in x)


_REF = {}


def reference(m1, m2, N, dt, theta, rates, grids4, U0, fix, ref_spot, mode, weights, strikes, put=True, div=None, scheme=0, N_i=None,
              dt_i=None, models=None, rows=None):
    """cliquet_ref.solve_batch, computed once per distinct input, shared and left unchanged.  grids4: (vs, vv, ds, dv)."""
    key = freeze((m1, m2, N, dt, theta, rates, grids4, U0, fix, ref_spot, mode, weights, strikes, put, div, scheme, N_i, dt_i, models, rows))
    if key not in _REF:
        U = QR.solve_batch(m1, m2, N, dt, theta, rates[0], rates[1], *MODEL, *grids4, U0, fix, ref_spot, np.asarray(mode), weights, None,
                           dividends=div, put_strikes=strikes if put else None, scheme=scheme, N_i=N_i, dt_i=dt_i, rows=rows, models=models)
        U.setflags(write=False)
        _REF[key] = U
    return _REF[key]
