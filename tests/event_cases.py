"""Shapes, live ranges and event schedules shared by the event-domain tests of the Bermudan exercise and the knock-out barrier
(tests/test_emu_event_domain.py on the CPU, tests/test_gpu_event_domain.py on the device).  Plain data and numpy helpers.

SHAPES walks the admitted domain of the event kernels, which visit SLOTS of the packed state, not nodes (hadi_core.h,
hadi_slot_to_i): every change of (B, G) in hadi_pick_shape has a row on either side of it, so rows hold odd and even numbers of
nodes; the v-axis rows sit on either side of the end of LDS admission (32 | 33 v-intervals), of a chunk count (33 | 34, 65 | 66,
263 | 264) and of the sequential column pass (527 | 528).  LDS_ROWS are the shapes of the whole-loop kernels.

live_ranges names the index ranges (ia, ib) a barrier pair can leave alive and returns barriers that realise each of them.
schedules_near_dividends returns event schedules placed against the paying steps of a dividend schedule.
"""
import collections

import numpy as np

import common as Cm
import dividend_schedules as D

S_AXIS_M1 = (16, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
# m2 -> m1 of the v-axis rows.  m2 = 33 and 66 take V_0 = 0.09 (Cm.v0_for), 34 and 65 take 0.04: the 33 | 34 and 65 | 66 pairs
# differ in the v-grid family as well as in the chunk count, so a failure on one side does not by itself point at the chunks.
V_AXIS = ((31, 40), (32, 65), (33, 40), (34, 65), (65, 40), (66, 40), (263, 40), (264, 65), (527, 40), (528, 40))
# (a layout has m2 + 1 v-rows in chunks of HADI_LC = 33: P = ceil((m2 + 1) / 33), identity rows up to 33 P)
V_AXIS_WHAT = {31: "32 v-rows: one chunk, one identity row", 32: "33 v-rows: one chunk exactly full; the last m2 the LDS kernels admit",
               33: "34 v-rows: two chunks, 32 identity rows", 34: "35 v-rows: two chunks, 31 identity rows",
               65: "66 v-rows: two chunks exactly full", 66: "67 v-rows: three chunks", 263: "264 v-rows: eight chunks exactly full",
               264: "265 v-rows: nine chunks", 527: "528 v-rows: sixteen chunks exactly full, the last chunked layout",
               528: "529 v-rows: hadi_pass_b_seq, one chunk of all rows and no identity row"}

Shape = collections.namedtuple("Shape", "name m1 m2 what")


def pick_shape(m1):
    """(B, G) of hadi_pick_shape (hadi_core.h): nodes per lane and wavefronts per row."""
    if m1 <= 64:
        return 1, 1
    if m1 <= 128:
        return 2, 1
    if m1 <= 256:
        return 4, 1
    if m1 <= 512:
        return 8, 1
    if m1 <= 1024:
        return 8, 2
    return 1, (m1 + 63) // 64


def _s_what(m1):
    B, G = pick_shape(m1)
    return "%d nodes per row (%s), B = %d, G = %d, %d of %d slots are nodes" % (m1 + 1, "odd" if m1 % 2 == 0 else "even", B, G, m1,
                                                                                  64 * B * G)


SHAPES = [Shape("s%d" % m1, m1, 16 if m1 in (64, 65) else 8, _s_what(m1)) for m1 in S_AXIS_M1] + \
         [Shape("v%d" % m2, m1, m2, V_AXIS_WHAT[m2]) for m2, m1 in V_AXIS]
# the whole-loop LDS kernels; a seventh row, 128 x the largest m2 the route admits, is found by the tests (never hard-coded).
# 64x32 has 33 v-rows: hadi_small_seq2_kernel holds at most 32, so small_pairs = 1 must run hadi_small_seq_kernel there.  (With two
# nodes per lane the LDS budget ends below that: 65x32 is a streaming shape -- the tests assert it -- and is the v32 row above.)
LDS_ROWS = [(16, 11), (63, 24), (64, 31), (64, 32), (127, 16), (128, 20)]
NOT_LDS = (65, 32)

_BATCH = {}


def oracle_batch(m1, m2, n):
    """(strikes, vs, vv, ds, dv, call payoff) of n well-conditioned instances (the 30x rule is asserted, never a filter), built
    once per shape and left unchanged."""
    if (m1, m2, n) not in _BATCH:
        strikes = Cm.well_conditioned_strikes(m1, n)
        g = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
        Cm.assert_well_conditioned(g[2], g[3])
        for a in g:
            a.setflags(write=False)
        _BATCH[(m1, m2, n)] = (strikes,) + g
    return _BATCH[(m1, m2, n)]


# ---- live ranges ----------------------------------------------------------------------------------------------------------------
REBATES = (1.5, 0.25, 3.0, 0.5, 2.0)  # non-zero, one per instance of a batch of five
Live = collections.namedtuple("Live", "name ia ib lower upper on_nodes")


def located(vec_s, lower, upper):
    """(ia, ib) by the inequalities of hadi.h: node i is alive when lower < s_i < upper; (m1 + 1, -1) when none is."""
    vec_s = np.asarray(vec_s, dtype=np.float64)
    alive = np.nonzero((vec_s > lower) & (vec_s < upper))[0]
    return (int(alive[0]), int(alive[-1])) if len(alive) else (len(vec_s), -1)


def live_ranges(vec_s, B, G, strike):
    """The target ranges of one instance's s-grid, each with barriers that realise it: alternately as midpoints between two
    nodes and exactly ON the last knocked nodes (touching knocks out, so the live range starts one node further in).  A side
    whose range reaches the end of the grid has no barrier (-inf / +inf).  c is the first node at or above the strike."""
    vs = np.asarray(vec_s, dtype=np.float64)
    m1 = len(vs) - 1
    c = int(np.searchsorted(vs, strike))
    assert 2 <= c <= m1 - 3, (c, m1)
    targets = [("node 0 only", 1, m1 - 1, True),  # lower = s_0 (the grid's 0, 1.4e-14 in fp64) exactly: on the node
               ("two from either end", 2, m1 - 2, False), ("no lower side", 0, m1 - 1, True), ("no upper side", 1, m1, False),
               ("width one", c, c, False), ("width two", c, c + 1, True), ("width three", c - 1, c + 1, False)]
    if G == 2:
        # (wavefront 0 owns nodes 1 .. 64 B; on 513 intervals wavefront 1 owns node 513 alone and the range ends with the grid)
        targets.append(("astride two wavefronts", 64 * B - 1, min(64 * B + 2, m1), True))
    out = []
    for name, ia, ib, on in targets:
        lower = -np.inf if ia == 0 else float(vs[ia - 1]) if on else 0.5 * float(vs[ia - 1] + vs[ia])
        upper = np.inf if ib == m1 else float(vs[ib + 1]) if on else 0.5 * float(vs[ib] + vs[ib + 1])
        assert located(vs, lower, upper) == (ia, ib), (name, ia, ib, located(vs, lower, upper))
        out.append(Live(name, ia, ib, lower, upper, on))
    assert out[0].lower == vs[0] and abs(vs[0]) < 1e-12
    return out


def barrier_batch(vec_s, strikes, turn=0):
    """(lower, upper, rebate, iab, names) of a batch: instance k takes range (k + turn) of its own grid's live_ranges.  iab is
    what hadi_barrier_locate_kernel must find, computed from the inequalities."""
    n, m1 = vec_s.shape[0], vec_s.shape[1] - 1
    B, G = pick_shape(m1)
    lo, up, iab, names = np.empty(n), np.empty(n), [], []
    for k in range(n):
        r = live_ranges(vec_s[k], B, G, strikes[k])
        pick = r[(k + turn) % len(r)]
        lo[k], up[k] = pick.lower, pick.upper
        iab.append(list(located(vec_s[k], pick.lower, pick.upper)))
        names.append(pick.name)
    return lo, up, np.array([REBATES[k % 5] for k in range(n)]), iab, names


def turn(row):
    """The turn of SHAPES[row]: steps of three, so that the three two-wavefront rows reach all eight ranges with three instances."""
    return 3 * row


def n_live_ranges(m1):
    return 8 if pick_shape(m1)[1] == 2 else 7


# ---- events next to dividends ---------------------------------------------------------------------------------------------------
# A case: its name, the sweep's (N, dt), the dividend schedule, the event steps, the name dividend_schedules.requirement knows the
# schedule by, and whether it is run on call and on put data.  `barrier`: None = the two-sided default of the caller; "floor" = a lower barrier that knocks node 0 (and a few more) with no
# upper side, so that a jump reading node 0 reads the rebate the previous monitoring step wrote there.
Near = collections.namedtuple("Near", "name N dt dividends events req barrier calls puts")


def schedules_near_dividends(N, dt, T):
    """The event schedules of the event-domain tests for a sweep of N steps of dt.  With the canonical dates (paying on 4, 8, 11,
    16 of 20 steps): events on the steps BEFORE the paying ones (event at the end of n, jump at the start of n + 1), on the paying
    steps themselves, and on every step.  From dividend_schedules.named: a jump on step 1 with an event at 1, a jump on the last
    step with events at N - 1 and N, the densest schedule with events on every step, and the jump's non-interpolating branches
    (nonpos: big_cash; fallback: zero, negative) right after a monitoring step.  check(case, vec_s) asserts what each is named
    for."""
    out = []
    canon = (list(Cm.DIVS[0]), list(Cm.DIVS[1]), list(Cm.DIVS[2]))
    paid = sorted(D.paying_steps(N, dt, canon[0]))
    if len(paid) >= 3 and paid[0] > 1:
        out += [Near("before the paying steps", N, dt, canon, [p - 1 for p in paid], "canon", None, True, True),
                Near("on the paying steps", N, dt, canon, paid, "canon", None, True, True),
                Near("every step", N, dt, canon, list(range(1, N + 1)), "canon", None, True, True)]
    s = D.named(N, dt, T)
    every = list(range(1, N + 1))
    out += [Near("step1", N, dt, s["step1"], [1], "step1", None, True, True),
            Near("lastN", N, dt, s["lastN"], [N - 1, N], "lastN", None, True, True),
            Near("alternate", N, dt, s["alternate"], every, "alternate", None, True, True),
            Near("big_cash", N, dt, s["big_cash"], [1, 2], "big_cash", "floor", True, False),
            Near("negative", N, dt, s["negative"], [1, 4], "negative", "floor", True, True),
            Near("zero", N, dt, s["zero"], [1], "zero", "floor", True, True)]
    return out


def check(case, vec_s):
    """Conditions on the inputs alone: the schedule reaches its branch (dividend_schedules.requirement) and the events stand
    where the case's name says, relative to the paying steps."""
    paid, counts = D.requirement(case.req, case.N, case.dt, case.dividends, vec_s)
    ev = set(case.events)
    if case.name == "before the paying steps":
        assert ev == {p - 1 for p in paid} and not ev & set(paid), (ev, paid)
    elif case.name == "on the paying steps":
        assert ev == set(paid)
    elif case.name == "step1":
        assert 1 in paid and 1 in ev
    elif case.name == "lastN":
        assert case.N in paid and {case.N - 1, case.N} <= ev
    elif case.name in ("every step", "alternate"):
        assert ev == set(range(1, case.N + 1)) and paid
    else:  # big_cash, negative, zero: a monitoring step ends right before every paying step begins
        assert all(p - 1 in ev for p in paid), (ev, paid)
    return paid, counts


def floor_barrier(vec_s, k=3):
    """A lower barrier midway between nodes k - 1 and k of every instance (nodes 0 .. k - 1 knocked), no upper side."""
    vs = np.asarray(vec_s, dtype=np.float64)
    return 0.5 * (vs[:, k - 1] + vs[:, k]), np.full(vs.shape[0], np.inf)
