"""CPU-only check of the Bermudan exercise and the knock-out barrier over their admitted domain, under the wave emulator
(tests/emu/emu_bermudan.cpp, tests/emu/emu_barrier.cpp).  tests/test_emu_bermudan.py and tests/test_emu_barrier.py run 50x25 and
100x20 with barriers at fractions of near-equal strikes; this file runs

  A. every row of event_cases.SHAPES on the streaming kernels (ring, strips, paired strips, the sequential row and column passes)
     and the LDS rows on the five whole-loop kernels: five instances on the live ranges of event_cases.live_ranges (width one, two,
     three, node 0 only, node m1 only, astride two wavefronts, barriers between nodes and ON nodes), monitored at [1, N]; a put
     exercised at [1, N].  The located (ia, ib) are compared with the table, and every element of the packed state that is no
     node (pad slots, slots of nodes beyond m1, identity rows) with the same run without events.
  B. the schedules of event_cases.schedules_near_dividends on every Douglas path of 50x25 and 100x20, call and put.

The reference is tests/bermudan_ref.py / tests/barrier_ref.py at this file family's bound, 1e-10 of the instance's max|U_ref|, on
well-conditioned grids (asserted)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import barrier_ref as KR
import bermudan_ref as BR
import common as Cm
import event_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH, STREAM = range(6)
NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch", STREAM: "streaming"}
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH = {0: Cm.THETA, 2: 1.0 / 3.0}
BER, BAR = "bermudan", "barrier"
NOT_ADMITTED = 3
# HadiRouteKind and the tail of the route's description (tests/test_emu_barrier.py)
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING = range(6)


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


def build(name):
    so = os.path.join(HERE, "emu", "libhadi_emu_%s.so" % name)
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_%s.cpp" % name, "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = "%s.tmp.%d" % (so, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp, os.path.join(HERE, "emu", "emu_%s.cpp" % name)])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    getattr(lib, "emu_%s_packed_size" % name).restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


@pytest.fixture(scope="module")
def emu():
    return {BER: build(BER), BAR: build(BAR)}


def schedule_array(ev):
    return np.asarray(ev, dtype=np.int32).reshape(1, -1)


class Run:
    """One batch on one shape: the inputs, the emulated run and the reference (computed once per distinct input and kept)."""
    _REF = {}

    def __init__(self, what, m1, m2, n, N, events, put, dt=None, div=None, bar=None, scheme=0):
        self.what, self.m1, self.m2, self.n, self.N, self.events, self.put, self.div, self.scheme = what, m1, m2, n, N, list(events), put, div, scheme
        self.dt = Cm.T / N if dt is None else dt
        self.strikes, self.vs, self.vv, self.ds, self.dv, call = E.oracle_batch(m1, m2, n)
        self.U0 = Cm.put_payoff(self.vs, self.strikes, m2) if put else call
        self.bar = bar

    def emulate(self, emu, kind, strip=None, events=None):
        """(field [n][m], packed state, mask of its non-node elements, located ranges or None); NOT_ADMITTED if refused."""
        lib, n, m1, m2 = emu[self.what], self.n, self.m1, self.m2
        par8 = np.array([list(MODEL) + [self.dt, self.N, self.strikes[k] if self.put else 0.0, 1.0 if self.put else 0.0] for k in range(n)])
        dd = [np.ascontiguousarray(x, dtype=np.float64) for x in self.div] if self.div else [None] * 3
        nd = len(self.div[0]) if self.div else 0
        a = schedule_array(self.events if events is None else events)
        n_ev = a.shape[1]
        Uout = np.zeros_like(self.U0)
        size = getattr(lib, "emu_%s_packed_size" % self.what)(n, m1, m2)
        assert size > 0
        P, pad, iab = np.zeros(size), np.zeros(size, dtype=np.uint8), np.zeros((n, 2), dtype=np.int32)
        head = (n, m1, m2, C.c_double(TH[self.scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(self.vs), _P(self.vv),
                _P(self.ds), _P(self.dv), _P(self.U0))
        if strip is not None:
            lib.emu_set_tuning(b"strip", strip)
        try:
            if self.what == BER:
                rc = lib.emu_bermudan_state(*head, None, kind, self.scheme, nd, _P(dd[0]), _P(dd[1]), _P(dd[2]), n_ev,
                                            a.ctypes.data_as(_ip), 1, _P(Uout), _P(P), pad.ctypes.data_as(C.c_void_p))
            else:
                lo, up, reb = (np.ascontiguousarray(x, dtype=np.float64) for x in self.bar)
                rc = lib.emu_barrier(*head, kind, self.scheme, nd, _P(dd[0]), _P(dd[1]), _P(dd[2]), _P(lo), _P(up), _P(reb), n_ev,
                                     a.ctypes.data_as(_ip), 1, _P(Uout), _P(P), pad.ctypes.data_as(C.c_void_p), iab.ctypes.data_as(_ip))
        finally:
            lib.emu_set_tuning(b"reset", 0)
        if rc == NOT_ADMITTED:
            return rc
        assert rc == 0, rc
        assert lib.emu_take_error() == 0
        return Uout, P, pad.astype(bool), iab if self.what == BAR else None

    def ref(self):
        key = (self.what, self.m1, self.m2, self.n, self.N, self.dt, tuple(self.events), self.put, self.scheme,
               None if self.div is None else tuple(map(tuple, self.div)), None if self.bar is None else tuple(x.tobytes() for x in self.bar))
        if key not in self._REF:
            head = (self.m1, self.m2, self.N, self.dt, TH[self.scheme], Cm.R_D, Cm.R_F) + MODEL + (self.vs, self.vv, self.ds, self.dv, self.U0,
                                                                                                     self.events)
            kw = dict(dividends=self.div, put_strikes=self.strikes if self.put else None, scheme=self.scheme)
            U = BR.solve_batch(*head, **kw) if self.what == BER else KR.solve_batch(*head, *self.bar, **kw)
            U.setflags(write=False)
            self._REF[key] = U
        return self._REF[key]

    def check(self, emu, name, kind, strip=None):
        got = self.emulate(emu, kind, strip)
        assert got != NOT_ADMITTED, (name, NAMES[kind])
        U, P, pad, iab = got
        Uo = self.ref()
        scale = np.abs(Uo).max(axis=1)
        assert (scale > 0).all()
        err = np.abs(U - Uo).max(axis=1) / scale
        print("%s %s %s %dx%d: %.2e of max|U_ref|" % (name, self.what, NAMES[kind], self.m1, self.m2, err.max()))
        assert np.isfinite(U).all() and err.max() <= 1e-10, (name, NAMES[kind], err)
        # what is no node: exactly what the same run leaves there without events
        _, P0, pad0, _ = self.emulate(emu, kind, strip, events=[])
        assert pad.any() and np.array_equal(pad, pad0) and np.array_equal(P[pad], P0[pad]), (name, NAMES[kind])
        return iab


def live_barrier_run(m1, m2, n, N, turn):
    strikes, vs = E.oracle_batch(m1, m2, n)[:2]
    lo, up, reb, iab, names = E.barrier_batch(vs, strikes, turn)
    return Run(BAR, m1, m2, n, N, [1, N], False, bar=(lo, up, reb)), iab


# ---- A. shapes ------------------------------------------------------------------------------------------------------------------
def streaming_rows():
    """(shape, strip tuning): the ring and the strips (paired strips where a row has two wavefronts) of every class that has
    strips; the plan's own kernels below 65 and above 1024 s-intervals."""
    out = []
    for k, s in enumerate(E.SHAPES):
        for strip in ((0, 1) if 64 < s.m1 <= 1024 else (None,)):
            out.append((k, s, strip))
    return out


STREAM_IDS = ["%s-%dx%d-%s" % (s.name, s.m1, s.m2, {None: "plan", 0: "ring", 1: "strips"}[strip]) for _, s, strip in streaming_rows()]


@pytest.mark.parametrize("k,s,strip", streaming_rows(), ids=STREAM_IDS)
def test_streaming_shapes_barrier_on_the_live_ranges(emu, k, s, strip):
    run, iab = live_barrier_run(s.m1, s.m2, 5, 2, E.turn(k))
    got = run.check(emu, s.name, STREAM, strip)
    assert got.tolist() == iab, (got.tolist(), iab)


@pytest.mark.parametrize("k,s,strip", streaming_rows(), ids=STREAM_IDS)
def test_streaming_shapes_bermudan_put(emu, k, s, strip):
    Run(BER, s.m1, s.m2, 3, 2, [1, 2], True).check(emu, s.name, STREAM, strip)


def test_the_live_ranges_are_all_reached():
    """Instance k of row r takes range k + turn(r): with three instances already, every range is somebody's in both classes."""
    seen = {}
    for r, s in enumerate(E.SHAPES):
        strikes, vs = E.oracle_batch(s.m1, s.m2, 5)[:2]
        seen.setdefault(E.pick_shape(s.m1)[1] == 2, set()).update(E.barrier_batch(vs, strikes, E.turn(r))[4][:3])
    assert len(seen[False]) == 7 and len(seen[True]) == 8, seen
    for s in E.SHAPES:  # the table itself: both kinds of barrier, widths 1, 2, 3, the ends of the grid
        strikes, vs = E.oracle_batch(s.m1, s.m2, 5)[:2]
        R = E.live_ranges(vs[0], *E.pick_shape(s.m1), strikes[0])
        assert len(R) == E.n_live_ranges(s.m1) and {r.on_nodes for r in R} == {True, False}
        assert {r.ib - r.ia for r in R} >= {0, 1, 2} and any(r.ia == 0 for r in R) and any(r.ib == s.m1 for r in R)
        assert all(np.isinf(r.lower) == (r.ia == 0) and np.isinf(r.upper) == (r.ib == s.m1) for r in R)


def route(emu, n, m1, m2, tuning="", scheme=0):
    arr = (C.c_int * 16)(256, n, m1, m2, 0, scheme, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0)
    o, subs, desc = (C.c_longlong * 16)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
    f = emu[BAR].emu_route_barrier
    f.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    assert f(arr, TH[scheme], tuning.encode(), 2, o, subs, 64, desc, 1024) == 0
    return o[1], desc.value.decode()


def largest_lds_m2(emu, m1):
    """The largest m2 at which the route still takes a whole-loop LDS kernel for three instances on m1 s-intervals."""
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
@pytest.mark.parametrize("what", [BER, BAR])
def test_lds_shapes(emu, what, row, kind, scheme):
    m1, m2 = lds_rows(emu)[row]
    assert route(emu, 3, m1, m2)[0] != STREAMING and (row < 6 or m2 >= 20)
    if what == BAR:
        run, iab = live_barrier_run(m1, m2, 5, 3, row)
        run.scheme = scheme
    else:
        run, iab = Run(BER, m1, m2, 5, 3, [1, 3], scheme == 0, scheme=scheme), None
    if kind == SEQ2 and m2 + 1 > 32:
        # the pairs kernel holds at most 32 v-rows: the entry refuses, and the route of small_pairs = 1 is the one-instance kernel
        assert run.emulate(emu, kind) == NOT_ADMITTED
        k, d = route(emu, 5, m1, m2, "small_seq=1,small_pairs=1")
        assert k == SMALL_SEQ and "hadi_small_seq_kernel<" in d and "seq2" not in d, d
        return
    got = run.check(emu, "lds", kind)
    assert iab is None or got.tolist() == iab, (got.tolist(), iab)


def test_two_nodes_per_lane_leave_the_lds_kernels_before_33_rows(emu):
    m1, m2 = E.NOT_LDS
    assert route(emu, 3, m1, m2)[0] == STREAMING and route(emu, 3, m1, m2, "small_seq=1,small_pairs=1")[0] == STREAMING
    assert largest_lds_m2(emu, m1) < m2 == largest_lds_m2(emu, 64)


# ---- B. events next to dividends ------------------------------------------------------------------------------------------------
DOUGLAS_PATHS = [(BLOCK4, None), (BLOCK8, None), (SEQ, None), (SEQ2, None), (STREAM, 0), (STREAM, 1)]
IDS = ["block4", "block8", "seq", "pairs", "ring", "strips"]
NEAR = E.schedules_near_dividends(20, Cm.T / 20, Cm.T)[:3] + E.schedules_near_dividends(10, Cm.T / 10, Cm.T)[-6:]
# (big_cash is the call's case: on the nonpos branch a put takes its s = 0 value, which is what the fallback cases read)
NEAR_PUT = [(c, p) for c in NEAR for p in (False, True) if (c.puts if p else c.calls)]
LOF, UPF = (0.7, 0.8, 0.6), (1.3, 1.2, 1.4)


def near_run(what, m1, m2, case, put):
    n = 3
    strikes, vs = E.oracle_batch(m1, m2, n)[:2]
    for k in range(n):
        E.check(case, vs[k])
    if case.barrier == "floor":
        bar = E.floor_barrier(vs) + (np.full(n, 2.0),)
    else:
        bar = (np.array(LOF) * strikes, np.array(UPF) * strikes, np.array(E.REBATES[:n]))
    return Run(what, m1, m2, n, case.N, case.events, put, dt=case.dt, div=case.dividends, bar=bar if what == BAR else None)


def test_the_near_cases_are_the_ones_named():
    assert [c.name for c in NEAR] == ["before the paying steps", "on the paying steps", "every step", "step1", "lastN", "alternate",
                                      "big_cash", "negative", "zero"]
    assert NEAR[0].events == [3, 7, 10, 15] and NEAR[1].events == [4, 8, 11, 16] and NEAR[2].events == list(range(1, 21))


@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
@pytest.mark.parametrize("case,put", NEAR_PUT, ids=["%s-%s" % (c.name.replace(" ", "_"), "put" if p else "call") for c, p in NEAR_PUT])
@pytest.mark.parametrize("what", [BER, BAR])
def test_events_next_to_dividends(emu, what, case, put, m1, m2):
    run = near_run(what, m1, m2, case, put)
    for (kind, strip), name in zip(DOUGLAS_PATHS, IDS):
        if strip == 1 and m1 <= 64:
            continue  # (one node per lane has no strip kernel: that run is the ring's)
        run.check(emu, case.name + " " + name, kind, strip)


def test_before_and_on_the_paying_steps_differ_in_the_reference():
    for what in (BER, BAR):
        for put in (False, True):
            a, b = near_run(what, 50, 25, NEAR[0], put).ref(), near_run(what, 50, 25, NEAR[1], put).ref()
            assert np.abs(a - b).max() / np.abs(a).max() >= 1e-4, (what, put)
