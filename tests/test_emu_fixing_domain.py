"""CPU-only check of the strike fixing over its admitted domain, under the wave emulator (tests/emu/emu_cliquet.cpp).
tests/test_emu_cliquet.py runs 50x25 and 100x20 -- even m1, one or two nodes per lane, one chunk of v-rows; this file runs

  A. every row of event_cases.SHAPES on the streaming kernels (ring, strips, paired strips, the sequential row and column passes)
     followed by hadi_fixing_gather_kernel and hadi_fixing_kernel, and the LDS rows on the five whole-loop kernels
     (hadi_fixing_lds): five instances on the placements of fixing_cases.reference_nodes, fixed at [1, N], put data, every
     instance with its own row of weights (zero and non-zero at N).  The located nodes and status words are compared with the
     table; every element of the packed state that is no node (pad slots, slots of nodes beyond m1, identity rows) with the same
     run without fixings, bit for bit; where the fixing at N has weight 0, SHARES keeps the bits of (i_ref, j) and RETURN makes
     row j equal c_j's bits.
  B. the schedules of fixing_cases.near_fixings on every Douglas path of 50x25 and 100x20, put and call.

and, on the reference alone (no emulator): the placements are all reached in every (B, G) class, every batch has a zero and a
non-zero weight at N, no reference field is a zero field, and a reference node off by one moves every instance's reference by
>= 1e-4 of its max|U_ref| -- so the 1e-10 bound below cannot be met with a neighbouring node.

The reference is tests/cliquet_ref.py at this file family's bound, 1e-10 of the instance's max|U_ref|, on well-conditioned grids
(asserted).  Put data throughout A: call data with a RETURN fixing at node 0 gives a field of max|U| ~ 1e-16, against which a
relative bound means nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cliquet_ref as QR
import common as Cm
import event_cases as E
import fixing_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_cliquet.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH, STREAM = range(6)
NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch", STREAM: "streaming"}
TH = {0: Cm.THETA, 2: 1.0 / 3.0}
RATES = (Cm.R_D, Cm.R_F)
SHARES, RETURN = F.SHARES, F.RETURN
NOT_ADMITTED = 3
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING = range(6)  # enum HadiRouteKind


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_cliquet.cpp", "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp, os.path.join(HERE, "emu", "emu_cliquet.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_cliquet_packed_size.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


def padded(rows, n, dtype):
    """The host array of the ABI: [rows][width], zero-padded; one list = one shared row."""
    if rows and np.ndim(rows[0]) == 1:
        a = np.zeros((n, max(1, max(len(r) for r in rows))), dtype=dtype)
        for k, r in enumerate(rows):
            a[k, :len(r)] = r
        return a
    return np.asarray(rows, dtype=dtype).reshape(1, -1)


class Run:
    """One batch on one shape: the inputs, the emulated run and the reference (computed once per distinct input and kept)."""

    def __init__(self, m1, m2, n, N, fix, weights, ref_spot, mode, i_ref, put=True, dt=None, div=None, scheme=0):
        self.m1, self.m2, self.n, self.N, self.fix, self.weights, self.put, self.div, self.scheme = m1, m2, n, N, fix, weights, put, div, scheme
        self.ref_spot, self.mode, self.i_ref = np.asarray(ref_spot, dtype=np.float64), list(mode), list(i_ref)
        self.dt = Cm.T / N if dt is None else dt
        self.strikes, self.vs, self.vv, self.ds, self.dv, call = E.oracle_batch(m1, m2, n)
        self.U0 = Cm.put_payoff(self.vs, self.strikes, m2) if put else call

    def emulate(self, emu, kind, strip=None, fixings=True):
        """(field [n][m], packed state, mask of its non-node elements, located nodes and status words [2][n]); NOT_ADMITTED if
        the entry refuses the kernel on this shape."""
        n, m1, m2 = self.n, self.m1, self.m2
        par8 = np.array([list(F.MODEL) + [self.dt, self.N, self.strikes[k] if self.put else 0.0, 1.0 if self.put else 0.0] for k in range(n)])
        dd = [np.ascontiguousarray(x, dtype=np.float64) for x in self.div] if self.div else [None] * 3
        nd = len(self.div[0]) if self.div else 0
        a = padded(self.fix if fixings else [], n, np.int32)
        n_fix = 0 if a.size == 0 else a.shape[1]
        w = np.ascontiguousarray(padded(self.weights, n, np.float64)) if fixings and self.weights is not None else None
        assert w is None or w.shape == a.shape
        md = np.ascontiguousarray(self.mode, dtype=np.int32)
        ref = np.ascontiguousarray(self.ref_spot)
        Uout = np.zeros_like(self.U0)
        size = emu.emu_cliquet_packed_size(n, m1, m2)
        assert size > 0
        P, pad, iref = np.zeros(size), np.zeros(size, dtype=np.uint8), np.zeros((2, n), dtype=np.int32)
        if strip is not None:
            emu.emu_set_tuning(b"strip", strip)
        try:
            rc = emu.emu_cliquet(n, m1, m2, C.c_double(TH[self.scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(self.vs),
                                 _P(self.vv), _P(self.ds), _P(self.dv), _P(self.U0), None, kind, self.scheme, nd, _P(dd[0]), _P(dd[1]),
                                 _P(dd[2]), _P(ref), md.ctypes.data_as(_ip), n_fix, a.ctypes.data_as(_ip), a.shape[0], _P(w), _P(Uout),
                                 _P(P), pad.ctypes.data_as(C.c_void_p), iref.ctypes.data_as(_ip))
        finally:
            emu.emu_set_tuning(b"reset", 0)
        if rc == NOT_ADMITTED:
            return rc
        assert rc == 0, rc
        assert emu.emu_take_error() == 0
        return Uout, P, pad.astype(bool), iref

    def ref(self, rows=None):
        return F.reference(self.m1, self.m2, self.N, self.dt, TH[self.scheme], RATES, (self.vs, self.vv, self.ds, self.dv), self.U0, self.fix,
                           self.ref_spot, self.mode, self.weights, self.strikes, self.put, self.div, self.scheme, rows=rows)

    def last_weight(self, k):
        """The weight instance k's fixing at N carries (None: it has none there)."""
        shared = not (self.fix and np.ndim(self.fix[0]) == 1)
        steps = self.fix if shared else self.fix[k]
        if self.N not in steps:
            return None
        w = self.weights if shared else self.weights[k]
        return 0.0 if self.weights is None else float(w[list(steps).index(self.N)])

    def check(self, emu, name, kind, strip=None):
        got = self.emulate(emu, kind, strip)
        assert got != NOT_ADMITTED, (name, NAMES[kind])
        U, P, pad, iref = got
        Uo = self.ref()
        scale = np.abs(Uo).max(axis=1)
        assert (scale >= 1e-3).all(), scale
        err = np.abs(U - Uo).max(axis=1) / scale
        print("%s %s %dx%d: %.2e of max|U_ref|" % (name, NAMES[kind], self.m1, self.m2, err.max()))
        assert np.isfinite(U).all() and err.max() <= 1e-10, (name, NAMES[kind], err)
        # the located nodes and their status words
        assert iref[0].tolist() == self.i_ref and not iref[1].any(), (iref.tolist(), self.i_ref)
        # what is no node: exactly what the same run leaves there without fixings
        _, P0, pad0, _ = self.emulate(emu, kind, strip, fixings=False)
        assert pad.any() and not pad.all() and np.array_equal(pad, pad0), (name, NAMES[kind])
        assert np.array_equal(P[pad].view(np.uint64), P0[pad].view(np.uint64)), (name, NAMES[kind], int((P[pad] != P0[pad]).sum()))
        return U, err.max()

    def check_exact_bits(self, emu, name, kind, U, strip=None):
        """Where the fixing at N has weight 0: the run whose schedule stops short of N leaves the field the event at N reads; SHARES
        keeps the bits of column i_ref, RETURN makes every node of row j equal c_j.  Returns the instances checked."""
        zero = [k for k in range(self.n) if self.last_weight(k) == 0.0]
        if not zero:
            return zero
        shared = not (self.fix and np.ndim(self.fix[0]) == 1)
        cut = lambda steps, w: ([s for s in steps if s != self.N], None if w is None else [x for s, x in zip(steps, w) if s != self.N])
        if shared:
            fix, wts = cut(self.fix, self.weights)
        else:
            both = [cut(self.fix[k], None if self.weights is None else self.weights[k]) for k in range(self.n)]
            fix, wts = [b[0] for b in both], None if self.weights is None else [b[1] for b in both]
        before = Run(self.m1, self.m2, self.n, self.N, fix, wts, self.ref_spot, self.mode, self.i_ref, self.put, self.dt, self.div, self.scheme)
        V = before.emulate(emu, kind, strip)[0]
        Ur, Vr = U.reshape(self.n, self.m2 + 1, self.m1 + 1), V.reshape(self.n, self.m2 + 1, self.m1 + 1)
        for k in zero:
            c = Vr[k][:, self.i_ref[k]]
            assert np.array_equal(Ur[k][:, self.i_ref[k]].view(np.uint64), c.view(np.uint64)), (name, k, "column i_ref")
            if self.mode[k] == RETURN:
                flat = np.repeat(c[:, None], self.m1 + 1, axis=1)
                assert np.array_equal(Ur[k].view(np.uint64), flat.view(np.uint64)), (name, k, np.nonzero((Ur[k] != flat).any(axis=0))[0])
            else:
                other = self.i_ref[k] - 1 if self.i_ref[k] > 1 else self.i_ref[k] + 1
                assert not np.array_equal(Ur[k][:, other], c), (name, k)
        return zero


def shape_run(m1, m2, n, N, turn, scheme=0):
    strikes, vs = E.oracle_batch(m1, m2, n)[:2]
    ref, mode, i_ref, names = F.fixing_batch(vs, turn)
    fix, w = F.shape_schedule(n, N)
    return Run(m1, m2, n, N, fix, w, ref, mode, i_ref, put=scheme == 0, scheme=scheme), names


# ---- conditions on the inputs and on the reference alone ------------------------------------------------------------------------
RUNS = F.streaming_runs()
RUN_IDS = [r[0] for r in RUNS]


def test_every_placement_is_reached_in_every_class():
    """By the first three instances of the runs already (the batch of the large shapes on the device), so by every larger one."""
    assert [r[0] for r in RUNS if "turn" not in r[0]] == \
        ["%s-%dx%d-%s" % (s.name, s.m1, s.m2, x) for s in E.SHAPES for x in (("ring", "strips") if 64 < s.m1 <= 1024 else ("plan",))]
    seen, want = {}, {}
    for sid, k, s, strip, turn in RUNS:
        cls = E.pick_shape(s.m1) if s.m1 <= 1024 else "natural"
        vs = E.oracle_batch(s.m1, s.m2, 5)[1]
        seen.setdefault(cls, set()).update(F.fixing_batch(vs[:3], turn)[3])
        names = {p[0] for p in F.reference_nodes(s.m1)}
        assert len(names) == F.n_reference_nodes(s.m1) and want.setdefault(cls, names) == names
    assert set(seen) == {(1, 1), (2, 1), (4, 1), (8, 1), (8, 2), "natural"}
    for cls in want:
        assert seen[cls] == want[cls], (cls, want[cls] - seen[cls])
    assert len(want[(8, 2)]) == 12 and len(want["natural"]) == 14 and len(want[(1, 1)]) == 10


def test_the_placements_are_the_special_slots():
    for s in E.SHAPES:
        B, G = E.pick_shape(s.m1)
        pl = {name: (i, mode) for name, i, mode in F.reference_nodes(s.m1)}
        assert pl["node 0"] == (0, RETURN) and pl["node 1"][0] == 1 and pl["node m1"][0] == s.m1 and pl["node m1 - 1"][0] == s.m1 - 1
        assert F.pos(B, G, 0) == 64 * B * G and F.pair_partner(s.m1, 0) is None
        if s.m1 % 2:  # an even number of nodes: the last one shares its pair with the slot of node m1 + 1
            other = F.slot_to_i(B, G, F.pos(B, G, s.m1) ^ 1)
            assert F.pair_partner(s.m1, s.m1) is None and (other == s.m1 + 1 or other == -1), (s.m1, other)
        else:
            assert F.pair_partner(s.m1, s.m1) == s.m1 - 1
        o, e = pl["odd half of a pair, RETURN"][0], pl["even half of a pair, SHARES"][0]
        assert o % 2 == 1 and e == o + 1 and F.pos(B, G, o) % 2 == 0 and F.pos(B, G, e) == F.pos(B, G, o) + 1
        assert pl["odd half of a pair, SHARES"] == (o, SHARES) and pl["even half of a pair, RETURN"] == (e, RETURN)
        if B > 1:  # the last node of lane 0 and the first of lane 1 sit in different pairs, 2 slots apart
            assert F.pos(B, G, B + 1) == 2 and F.pos(B, G, B) == (B // 2 - 1) * 128 * G + 1
        if G == 2:
            assert F.pos(B, G, 64 * B + 1) == 128 and F.pos(B, G, 64 * B) < 128 * G * (B // 2) and "last node of wavefront 0" in pl
    # the odd-m1 rows exist on either side of every change of (B, G)
    assert {s.m1 for s in E.SHAPES if s.m1 % 2} >= {63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025}


def test_every_batch_has_a_zero_and_a_non_zero_weight_at_N():
    for n, N in ((3, 2), (5, 2), (5, 3)):
        fix, w = F.shape_schedule(n, N)
        assert all(r == [1, N] for r in fix) and any(r[1] == 0.0 for r in w) and any(r[1] != 0.0 for r in w)
    # node 0 with weight 0 at N -- the single store next to a pad, bits kept -- in every class, and on every odd-m1 row a RETURN
    # placement with weight 0 (the whole row, its half-filled last pair included, must be c_j's bits)
    node0, flat = set(), set()
    for sid, k, s, strip, turn in RUNS:
        vs = E.oracle_batch(s.m1, s.m2, 5)[1]
        _, mode, i_ref, _ = F.fixing_batch(vs, turn)
        w = F.shape_schedule(5, 2)[1]
        cls = E.pick_shape(s.m1) if s.m1 <= 1024 else "natural"
        if any(i_ref[q] == 0 and w[q][1] == 0.0 for q in range(5)):
            node0.add(cls)
        if any(mode[q] == RETURN and w[q][1] == 0.0 for q in range(5)):
            flat.add(s.m1)
    assert node0 == {(1, 1), (2, 1), (4, 1), (8, 1), (8, 2), "natural"}, node0
    assert flat >= {s.m1 for s in E.SHAPES if s.m1 % 2}, flat


def condition_batches(s):
    """The (n, N) a row runs with: five instances and two steps under the emulator (of which the device's three are the first
    three), and five instances and three steps on the small shapes of the device."""
    return [(5, 2)] + ([(5, 3)] if s.m1 <= 129 and s.m2 <= 66 else [])


@pytest.mark.parametrize("sid,k,s,strip,turn", RUNS, ids=RUN_IDS)
def test_no_zero_field_and_a_node_off_by_one_moves_the_reference(sid, k, s, strip, turn):
    """Conditions, not filters: every instance of every run.  max|U_ref| >= 1e-3, and the reference with i_ref - 1 and with
    i_ref + 1 (whichever exist) differs from the case's by >= 1e-4 of the instance's max|U_ref|."""
    for n, N in condition_batches(s):
        run, names = shape_run(s.m1, s.m2, n, N, turn)
        Uo = run.ref()
        scale = np.abs(Uo).max(axis=1)
        assert (scale >= 1e-3).all(), (names, scale)
        for q in range(n):
            for other in (run.i_ref[q] - 1, run.i_ref[q] + 1):
                if other < 0 or other > s.m1 or (other == 0 and run.mode[q] == SHARES):
                    continue
                V = QR.solve_one(s.m1, s.m2, N, run.dt, Cm.THETA, Cm.R_D, Cm.R_F, *F.MODEL, run.vs[q], run.vv[q], run.ds[q], run.dv[q],
                                 run.U0[q], run.fix[q], mode=run.mode[q], weights=run.weights[q], put_strike=run.strikes[q], i_ref=other)
                moved = np.abs(V - Uo[q]).max() / scale[q]
                assert moved >= 1e-4, (names[q], run.i_ref[q], other, moved)


@pytest.mark.parametrize("m1,m2", F.REGIME_SHAPES, ids=["%dx%d" % s for s in F.REGIME_SHAPES])
@pytest.mark.parametrize("rid", F.REGIMES)
def test_every_regime_moves_the_reference(rid, m1, m2):
    """The regimes the device runs with fixings (R0, R6: rates; T3, T5: theta and dt), three put instances fixing around their
    strikes: each differs from its canonical twin (same N, same fixings) by >= 1e-6 of max|U|, instance by instance, and is no
    zero field -- so a kernel on the wrong rate, theta or dt cannot pass."""
    rates, theta, dt, N, fix, canon = F.regime_inputs(rid)
    strikes, vs, vv, ds, dv, _ = E.oracle_batch(m1, m2, 3)
    ref, mode, i_ref = F.strike_batch(vs, strikes)
    U0 = Cm.put_payoff(vs, strikes, m2)
    w = F.mixed_weights(fix)
    Uo = F.reference(m1, m2, N, dt, theta, rates, (vs, vv, ds, dv), U0, fix, ref, mode, w, strikes)
    Uc = F.reference(m1, m2, N, canon["dt"], canon["theta"], tuple(canon["rates"]), (vs, vv, ds, dv), U0, fix, ref, mode, w, strikes)
    moved = np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)
    assert moved.min() >= 1e-6 and (np.abs(Uo).max(axis=1) >= 1e-3).all(), moved


# ---- A. shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid,k,s,strip,turn", RUNS, ids=RUN_IDS)
def test_streaming_shapes(emu, sid, k, s, strip, turn):
    run, names = shape_run(s.m1, s.m2, 5, 2, turn)
    U, _ = run.check(emu, "%s %s" % (s.name, names), STREAM, strip)
    zero = run.check_exact_bits(emu, s.name, STREAM, U, strip)
    assert len(zero) == 2


def route(emu, n, m1, m2, tuning="", scheme=0):
    arr = (C.c_int * 16)(256, n, m1, m2, 0, scheme, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0)
    o, subs, desc = (C.c_longlong * 17)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
    emu.emu_route_cliquet.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p,
                                      C.c_int]
    assert emu.emu_route_cliquet(arr, TH[scheme], tuning.encode(), 2, 1, o, subs, 64, desc, 1024) == 0
    return o[1], desc.value.decode()


def largest_lds_m2(emu, m1):
    """The largest m2 at which the route of a cliquet call still takes a whole-loop LDS kernel for three instances."""
    lds = [m2 for m2 in range(4, 129) if route(emu, 3, m1, m2)[0] in (SMALL, SMALL_SEQ, SMALL_SEQ2)]
    assert lds and lds == list(range(4, lds[-1] + 1)) and route(emu, 3, m1, lds[-1] + 1)[0] == STREAMING, lds
    return lds[-1]


LDS_KINDS = [(BLOCK4, 0), (BLOCK8, 0), (SEQ, 0), (SEQ2, 0), (SCH, 2)]
LDS_IDS = ["block4", "block8", "seq", "pairs", "sch-MCS"]
_LDS_MAX = {}


def lds_rows(emu):
    if 128 not in _LDS_MAX:
        _LDS_MAX[128] = largest_lds_m2(emu, 128)
    return E.LDS_ROWS + [(128, _LDS_MAX[128])]


@pytest.mark.parametrize("kind,scheme", LDS_KINDS, ids=LDS_IDS)
@pytest.mark.parametrize("row", range(7), ids=["%dx%d" % r for r in E.LDS_ROWS] + ["128xmax"])
def test_lds_shapes(emu, row, kind, scheme):
    """The scheme kernel on call data (the schemes' reference is the call's): its batch starts one placement on, so that no
    instance is RETURN at node 0, where call data give a zero field."""
    m1, m2 = lds_rows(emu)[row]
    assert route(emu, 3, m1, m2)[0] != STREAMING and (row < 6 or m2 >= 20)
    run, names = shape_run(m1, m2, 5, 3, row if scheme == 0 else 1, scheme)
    assert scheme == 0 or 0 not in run.i_ref
    if kind == SEQ2 and m2 + 1 > 32:
        # the pairs kernel holds at most 32 v-rows: the entry refuses, and the route of small_pairs = 1 is the one-instance kernel
        assert run.emulate(emu, kind) == NOT_ADMITTED
        k, d = route(emu, 5, m1, m2, "small_seq=1,small_pairs=1")
        assert k == SMALL_SEQ and "hadi_small_seq_kernel<" in d and "seq2" not in d, d
        return
    U, _ = run.check(emu, "lds %s" % names, kind)
    assert len(run.check_exact_bits(emu, "lds", kind, U)) == 2


def test_two_nodes_per_lane_leave_the_lds_kernels_before_33_rows(emu):
    m1, m2 = E.NOT_LDS
    assert route(emu, 3, m1, m2)[0] == STREAMING and route(emu, 3, m1, m2, "small_seq=1,small_pairs=1")[0] == STREAMING
    assert largest_lds_m2(emu, m1) < m2 == largest_lds_m2(emu, 64)


# ---- B. fixings next to dividends -----------------------------------------------------------------------------------------------
DOUGLAS_PATHS = [(BLOCK4, None), (BLOCK8, None), (SEQ, None), (SEQ2, None), (STREAM, 0), (STREAM, 1)]
IDS = ["block4", "block8", "seq", "pairs", "ring", "strips"]
NEAR = E.schedules_near_dividends(20, Cm.T / 20, Cm.T)[:3] + E.schedules_near_dividends(10, Cm.T / 10, Cm.T)[-6:]
# (big_cash is the call's case: on the nonpos branch a put takes its s = 0 value, which is what the fallback cases read)
NEAR_PUT = [(c, p) for c in NEAR for p in (False, True) if (c.puts if p else c.calls)]
NEAR_IDS = ["%s-%s" % (c.name.replace(" ", "_"), "put" if p else "call") for c, p in NEAR_PUT]


def near_run(m1, m2, case, put):
    strikes, vs = E.oracle_batch(m1, m2, 3)[:2]
    for k in range(3):
        E.check(case, vs[k])
    fix, w, ref, mode, i_ref = F.near_fixings(case, vs, strikes)
    return Run(m1, m2, 3, case.N, fix, w, ref, mode, i_ref, put=put, dt=case.dt, div=case.dividends)


def test_the_near_cases_are_the_ones_named():
    assert [c.name for c in NEAR] == ["before the paying steps", "on the paying steps", "every step", "step1", "lastN", "alternate",
                                      "big_cash", "negative", "zero"]
    assert NEAR[0].events == [3, 7, 10, 15] and NEAR[1].events == [4, 8, 11, 16] and NEAR[2].events == list(range(1, 21))
    assert [c.name for c in NEAR if c.barrier == "floor"] == ["big_cash", "negative", "zero"]
    for c in NEAR[-3:]:
        run = near_run(50, 25, c, c.puts)
        assert run.i_ref[:2] == [0, 1] and run.mode[:2] == [RETURN, SHARES] and 2 < run.i_ref[2] < 50


@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_before_and_on_the_paying_steps_differ_in_the_reference(m1, m2):
    for put in (False, True):
        a, b = near_run(m1, m2, NEAR[0], put).ref(), near_run(m1, m2, NEAR[1], put).ref()
        assert (np.abs(a).max(axis=1) >= 1e-3).all()
        assert np.abs(a - b).max() / np.abs(a).max() >= 1e-4, put


@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
@pytest.mark.parametrize("case,put", NEAR_PUT, ids=NEAR_IDS)
def test_fixings_next_to_dividends(emu, case, put, m1, m2):
    """Call data only where no instance's reference is a zero field (asserted by check: max|U_ref| >= 1e-3 for every instance)."""
    run = near_run(m1, m2, case, put)
    for (kind, strip), name in zip(DOUGLAS_PATHS, IDS):
        if strip == 1 and m1 <= 64:
            continue  # (one node per lane has no strip kernel: that run is the ring's)
        run.check(emu, case.name + " " + name, kind, strip)
