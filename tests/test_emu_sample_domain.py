"""CPU-only walk of the sampled ladder's admitted domain under the wave emulator (tests/emu/emu_samples.cpp): shapes, sample
counts and spot placements of tests/sample_cases.py.  tests/test_emu_samples.py runs 50x25 with ten spots per instance; this file

  A. runs the five whole-loop kernels (block4, block8, seq, pairs, sch-MCS) on every row of LDS_ROWS and on 50x25 -- B = 1 and
     B = 2, 16 to 129 nodes per row, 33 v-rows where the pairs kernel must refuse -- with domain_spots at full budget, and at 50x25
     and 128x20 at every entry of COUNTS into a buffer prefilled with a sentinel and followed by a guard tail;
  B. runs hadi_sample_locate_kernel, hadi_pack_kernel and hadi_sample_kernel on every row of event_cases.SHAPES (every (B, G),
     every chunk count) on a synthetic field, five instances in sub-batches of 3 + 2, V_0_i on rotated v-rows;
  C. pins the locate kernel on sample_cases.LOCATE_EDGES (m1 = 2 and 3, nodes closer than the tolerance, equal nodes, non-finite
     spots, signed zeros), whose expectations are written out by hand from include/hadi.h.

Checks: the tight check of sample_cases (interior samples against the node-hit columns of the same call, 32 * 2^-53 sum|w u| |scale|,
derived there); node-hit columns -- and, at the existing bound 1e-10 sum|w| |scale| max|U_ref|, every sample -- against samples_ref
applied to oracle fields at N = snap_steps[q]; the S_0 column against emu_ladder bit for bit.  Worst tight-check ratio measured
here: 0.130 of the bound on the whole-loop kernels, 0.142 on the streaming rows (DESIGN.md lists it per file, with the mutations
this file catches: six that tests/test_emu_samples.py misses)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import dividend_schedules as D
import sample_cases as SC
import samples_ref as R
import scheme_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_samples.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH = range(5)
NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch-MCS"}
KINDS = [BLOCK4, BLOCK8, SEQ, SEQ2, SCH]
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS = 1.0 / 3.0
N_INST, N_STEPS, SNAPS = 3, 4, [1, 3, 4]
NOT_ADMITTED = 3
SENTINEL, GUARD = -7.25e300, 4096
LOOP_ROWS = SC.LDS_ROWS + [(50, 25)]


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_samples.cpp", "emu_ladder.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (tests/test_emu_samples.py builds the same file: each moves a whole one into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp, os.path.join(HERE, "emu", "emu_samples.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_set_tuning(b"reset", 0)
    return lib


WORST = {"loop": 0.0, "stream": 0.0}


# ---- A. the whole-loop kernels --------------------------------------------------------------------------------------------------
class Loop:
    """One problem on one shape: three instances, N = 4, snapshots [1, 3, 4]; the oracle's fields computed once and kept."""
    _REF, _LAD = {}, {}

    def __init__(self, m1, m2, variant=0, scheme=0, put=False, divs=None, N=N_STEPS, snaps=SNAPS):
        self.m1, self.m2, self.variant, self.scheme, self.put, self.divs, self.N, self.snaps = m1, m2, variant, scheme, put, divs, N, list(snaps)
        self.theta = TH_MCS if scheme == 2 else Cm.THETA
        self.strikes, self.vs, self.vv, self.ds, self.dv, call = SC.oracle_batch(m1, m2, N_INST)
        self.U0 = Cm.put_payoff(self.vs, self.strikes, m2) if put else call
        self.v0 = Cm.v0_for(m2)
        self.dt = Cm.T / N
        self.par8 = np.array([list(MODEL) + [self.dt, N, self.strikes[k] if put else 0.0, 1.0 if put else 0.0] for k in range(N_INST)])
        self.key = (m1, m2, variant, scheme, put, divs is not None, N, tuple(snaps))

    def _head(self):
        dd = [np.ascontiguousarray(x, dtype=np.float64) for x in self.divs] if self.divs else [None] * 3
        self._keep = dd
        return (N_INST, self.m1, self.m2, C.c_double(self.theta), C.c_double(Cm.R_D), C.c_double(0.0), _P(self.par8), _P(self.vs), _P(self.vv),
                _P(self.ds), _P(self.dv), _P(self.U0), _P(self.U0)), (len(dd[0]) if self.divs else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]))

    def samples(self, emu, kind, spots, scales):
        """(out [n][n_snap][n_samp], flags) -- the buffer prefilled with a sentinel, its guard tail asserted untouched -- or
        NOT_ADMITTED."""
        head, div = self._head()
        n_samp = spots.shape[1]
        total = N_INST * len(self.snaps) * n_samp
        buf = np.full(total + GUARD, SENTINEL)
        flags = np.full((N_INST, n_samp), -1, dtype=np.int32)
        snaps = np.ascontiguousarray(self.snaps, dtype=np.int32)
        sp, sc = np.ascontiguousarray(spots), np.ascontiguousarray(scales)
        rc = emu.emu_samples(*head, kind, self.variant, self.scheme if kind == SCH else 0, *div, C.c_double(self.v0), n_samp, _P(sp), _P(sc),
                             N_INST, len(self.snaps), snaps.ctypes.data_as(_ip), _P(buf), flags.ctypes.data_as(_ip))
        if rc == NOT_ADMITTED:
            return rc
        assert rc == 0 and emu.emu_take_error() == 0, rc
        assert (buf[total:] == SENTINEL).all(), "written beyond n * n_snap * n_samp"
        assert not (buf[:total] == SENTINEL).any(), ("entries never written", np.argwhere(buf[:total] == SENTINEL)[:8].ravel())
        return buf[:total].reshape(N_INST, len(self.snaps), n_samp), flags

    def ladder(self, emu, kind):
        if (self.key, kind) not in self._LAD:
            head, div = self._head()
            snaps = np.ascontiguousarray(self.snaps, dtype=np.int32)
            out, status = np.full((N_INST, len(self.snaps)), np.nan), np.full(N_INST, -1, dtype=np.int32)
            rc = emu.emu_ladder(*head, kind, self.variant, self.scheme if kind == SCH else 0, *div, C.c_double(Cm.S_0), C.c_double(self.v0),
                                len(self.snaps), snaps.ctypes.data_as(_ip), _P(out), None, status.ctypes.data_as(_ip))
            assert rc == 0 and (status == 0).all()
            self._LAD[(self.key, kind)] = out
        return self._LAD[(self.key, kind)]

    def rows_of_v0(self, nq):
        """The oracle's row of V_0 after nq steps, [n][m1 + 1]: computed once per problem and step, left unchanged."""
        if (self.key, nq) not in self._REF:
            ovar = {0: O.EU, 1: O.AM, 2: O.DIV, 3: O.AM_DIV}[self.variant]
            rows, top = [], []
            for k in range(N_INST):
                if self.scheme:
                    p = O.make_params(self.m1, self.m2, nq, self.dt, self.theta, Cm.R_D, 0.0, *MODEL, O.EU)
                    U = S.solve_one(p, self.vs[k], self.vv[k], self.ds[k], self.dv[k], self.U0[k], {1: S.CS, 2: S.MCS, 3: S.HV}[self.scheme])
                else:
                    p = O.make_params(self.m1, self.m2, nq, self.dt, self.theta, Cm.R_D, 0.0, *MODEL, ovar, self.divs if self.variant & 2 else None,
                                      option_type=O.PUT if self.put else O.CALL, strikes=self.strikes[k] if self.put else None)
                    U = O.solve(p, self.vs[k], self.vv[k], self.ds[k], self.dv[k], self.U0[k], self.U0[k] if self.variant & 1 else None)[0]
                j0 = R.row_index(self.vv[k], self.v0)
                rows.append(np.array(U[j0 * (self.m1 + 1):(j0 + 1) * (self.m1 + 1)]))
                top.append(np.abs(U).max())
            self._REF[(self.key, nq)] = (np.stack(rows), np.array(top))
        return self._REF[(self.key, nq)]

    def check(self, emu, kind, count=None):
        spots, scales, kinds = SC.batch_spots(self.vs, Cm.S_0, 1024, count)
        got = self.samples(emu, kind, spots, scales)
        assert got != NOT_ADMITTED, (self.key, NAMES[kind])
        out, flags = got
        name = "%dx%d %s count %s" % (self.m1, self.m2, NAMES[kind], count)
        assert (flags == 0).all(), name
        assert np.array_equal(out[:, :, 0], self.ladder(emu, kind)), name  # the S_0 column is the ladder, bit for bit
        worst, checked = SC.tight_check(out, self.vs, spots, scales, name)
        assert checked == int(((kinds == SC.INTERIOR) | (kinds == SC.TOL_INTERIOR)).sum()), name
        # every sample against the oracle at the existing bound (a node hit: sum|w| = 1, so 1e-10 max|U_ref|)
        idx, w = SC.stencils(self.vs, spots)
        for q, nq in enumerate(self.snaps):
            rows, top = self.rows_of_v0(nq)
            u = np.stack([rows[k][idx[k]] for k in range(N_INST)])
            ref = (w * u).sum(axis=-1) * scales
            bound = 1e-10 * np.abs(w).sum(axis=-1) * np.abs(scales) * top[:, None]
            diff = np.abs(out[:, q, :] - ref)
            assert (diff <= bound).all(), (name, nq, np.argwhere(diff > bound)[:4], (diff / bound).max())
        WORST["loop"] = max(WORST["loop"], worst)
        print("%s: %d samples, %d interior, tight |diff| / bound %.3f (file so far %.3f)" % (name, spots.shape[1], checked // N_INST, worst,
                                                                                              WORST["loop"]))
        return worst


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: NAMES[k])
@pytest.mark.parametrize("m1,m2", LOOP_ROWS, ids=["%dx%d" % r for r in LOOP_ROWS])
def test_lds_shapes_at_full_budget(emu, m1, m2, kind):
    run = Loop(m1, m2, scheme=2 if kind == SCH else 0)
    if kind == SEQ2 and m2 + 1 > 32:  # the pairs kernel holds at most 32 v-rows: refused, as documented
        spots, scales, _ = SC.batch_spots(run.vs, Cm.S_0, 1024)
        assert run.samples(emu, kind, spots, scales) == NOT_ADMITTED
        return
    run.check(emu, kind)


def test_the_full_budget_lists_hold_what_they_are_named_for():
    """Conditions on the inputs: every interval of an LDS row three times, every node a hit, the tolerance block whole."""
    for m1, m2 in LOOP_ROWS:
        vs = SC.oracle_batch(m1, m2, N_INST)[1]
        spots, scales, kinds = SC.batch_spots(vs, Cm.S_0, 1024)
        assert 4 * m1 + 16 <= 1024 and spots.shape[1] <= 4 * m1 + 16
        for k in range(N_INST):
            assert (kinds[k] == SC.INTERIOR).sum() >= 3 * m1 and (kinds[k] == SC.TOL_HIT).sum() == 5 and (kinds[k] == SC.TOL_INTERIOR).sum() == 2
            assert {float(x) for x in spots[k][kinds[k] == SC.HIT]} == {float(x) for x in vs[k]}  # every node is a hit column
            assert (scales[k][kinds[k] <= SC.HIT] == 1.0).all() and (scales[k][kinds[k] == SC.INTERIOR] < 0).any()
            assert spots[k][0] == Cm.S_0 and 0.0 in spots[k] and vs[k][0] > 0.0 and vs[k][0] < 1e-13


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: NAMES[k])
@pytest.mark.parametrize("m1,m2", [(50, 25), (128, 20)], ids=["50x25", "128x20"])
def test_every_sample_count(emu, m1, m2, kind):
    """Every entry of COUNTS: the loops of hadi_sample_lds run zero, one and several times per lane on every stride (32, 64, 256,
    512); no entry keeps the sentinel and nothing is written beyond n * n_snap * n_samp (Loop.samples)."""
    run = Loop(m1, m2, scheme=2 if kind == SCH else 0)
    for count in SC.COUNTS:
        run.check(emu, kind, count)


@pytest.mark.parametrize("kind", [BLOCK4, BLOCK8], ids=lambda k: NAMES[k])
def test_american_on_the_block_kernels(emu, kind):
    run = Loop(127, 16, variant=1, put=True)
    if run.samples(emu, kind, *SC.batch_spots(run.vs, Cm.S_0, 1024)[:2]) == NOT_ADMITTED:
        run = Loop(50, 25, variant=1, put=True)  # (the American kernels' LDS budget ends earlier)
    run.check(emu, kind)


def _paying_steps(emu, N, dt):
    dates = np.ascontiguousarray(Cm.DIVS[0], dtype=np.float64)
    flags = np.full(N, -1, dtype=np.int32)
    emu.emu_dividend_steps(N, C.c_double(dt), len(dates), _P(dates), flags.ctypes.data_as(_ip), N)
    return [q + 1 for q in range(N) if flags[q] >= 0]


@pytest.mark.parametrize("kind", [BLOCK4, SEQ, SEQ2], ids=lambda k: NAMES[k])
def test_dividends_with_a_snapshot_on_a_paying_step_at_128x20(emu, kind):
    N, snaps = 10, [2, 4, 10]  # (snapshots on two paying steps and on one that pays nothing)
    assert _paying_steps(emu, N, Cm.T / N) == sorted(D.paying_steps(N, Cm.T / N, Cm.DIVS[0])) == [2, 4, 8]
    Loop(128, 20, variant=2, divs=Cm.DIVS, N=N, snaps=snaps).check(emu, kind)


# ---- B. the streaming path's locate, pack and gather on every layout ---------------------------------------------------------
def sample_field(emu, m1, m2, vs, vv, v0, v0_i, fields, spots, scales, sub):
    n, n_samp, n_snap = vs.shape[0], spots.shape[1], fields.shape[0]
    total = n * n_snap * n_samp
    buf = np.full(total + GUARD, SENTINEL)
    flags = np.full((n, n_samp), -1, dtype=np.int32)
    subs = np.ascontiguousarray(sub, dtype=np.int32)
    sp, sc = np.ascontiguousarray(spots), None if scales is None else np.ascontiguousarray(scales)
    v0i = None if v0_i is None else np.ascontiguousarray(v0_i, dtype=np.float64)
    rc = emu.emu_sample_field(m1, m2, n, _P(np.ascontiguousarray(vs)), _P(np.ascontiguousarray(vv)), C.c_double(v0), _P(v0i),
                              _P(np.ascontiguousarray(fields)), _P(sp), _P(sc), spots.shape[0], n_samp, n_snap, subs.ctypes.data_as(_ip),
                              len(sub), _P(buf), flags.ctypes.data_as(_ip))
    assert rc == 0, rc
    assert (buf[total:] == SENTINEL).all(), "written beyond n * n_snap * n_samp"
    return buf[:total].reshape(n, n_snap, n_samp), flags


@pytest.mark.parametrize("count", [257, 1024])
@pytest.mark.parametrize("s", SC.SHAPES, ids=["%s-%dx%d" % (s.name, s.m1, s.m2) for s in SC.SHAPES])
def test_streaming_shapes_on_a_synthetic_field(emu, s, count):
    n, m1, m2 = 5, s.m1, s.m2
    _, vs, vv, _, _, _ = SC.oracle_batch(m1, m2, n)
    lay = (C.c_int * 4)()
    assert emu.emu_sample_layout(m1, m2, n, lay) == 0 and (lay[0], lay[1]) == SC.pick_shape(m1)
    spots, scales, kinds = SC.batch_spots(vs, Cm.S_0, count, count)
    assert spots.shape == (n, count) and (kinds == SC.INTERIOR).sum(axis=1).min() >= 16
    # V_0_i on rotated v-rows; instance 2's is off its v-grid: row 0
    jrow = [(3 * k + 1) % (m2 + 1) for k in range(n)]
    v0_i = np.array([vv[k][jrow[k]] for k in range(n)])
    v0_i[2] = 0.0123456
    assert np.abs(vv[2] - v0_i[2]).min() > 1e-6
    jrow[2] = 0
    assert [R.row_index(vv[k], v0_i[k]) for k in range(n)] == jrow and len(set(jrow)) >= 3
    base = SC.synthetic_field(m1, m2, n)
    fields = np.stack([base, base + 2.0 ** 27])  # two snapshots
    out, flags = sample_field(emu, m1, m2, vs, vv, 0.5, v0_i, fields, spots, scales, [3, 2])
    assert (flags == 0).all() and not (out == SENTINEL).any()
    idx, w = SC.stencils(vs, spots)
    worst = 0.0
    for q in range(2):
        for k in range(n):
            u = fields[q, k, jrow[k] * (m1 + 1):(jrow[k] + 1) * (m1 + 1)][idx[k]]  # [n_samp][4]
            hit = idx[k, :, 0] == idx[k, :, 3]
            assert np.array_equal(out[k, q, hit], u[hit, 0] * scales[k, hit]), (s.name, k, q)  # node hits: bit for bit
            wi, ui, ci = w[k, ~hit], u[~hit], scales[k, ~hit]
            ref = ((((wi[:, 0] * ui[:, 0]) + wi[:, 1] * ui[:, 1]) + wi[:, 2] * ui[:, 2]) + wi[:, 3] * ui[:, 3]) * ci
            bound = SC.TIGHT * np.abs(wi * ui).sum(axis=1) * np.abs(ci)
            diff = np.abs(out[k, q, ~hit] - ref)
            assert (diff <= bound).all(), (s.name, k, q, np.argwhere(diff > bound)[:4].ravel(), (diff / bound).max())
            worst = max(worst, (diff / bound).max())
    WORST["stream"] = max(WORST["stream"], worst)
    print("%s %dx%d count %d: tight |diff| / bound %.3f (file so far %.3f)" % (s.name, m1, m2, count, worst, WORST["stream"]))


def test_sub_batches_write_what_one_batch_writes(emu):
    """The o * n_samp arithmetic: 3 + 2, 1 + 4, 2 + 2 + 1 and 5 give the same bits; n_samp odd, so no offset is a multiple of 256."""
    n, m1, m2 = 5, 300, 20
    _, vs, vv, _, _, _ = SC.oracle_batch(m1, m2, n)
    spots, scales, _ = SC.batch_spots(vs, Cm.S_0, 257, 257)
    fields = np.stack([SC.synthetic_field(m1, m2, n)] * 3) * np.array([1.0, 2.0, 4.0]).reshape(3, 1, 1)
    one, _ = sample_field(emu, m1, m2, vs, vv, Cm.v0_for(m2), None, fields, spots, scales, [5])
    assert len({one[k, q, 0] for k in range(n) for q in range(3)}) == 15  # every (instance, snapshot) differs in the S_0 column
    for sub in ([3, 2], [1, 4], [2, 2, 1]):
        assert np.array_equal(sample_field(emu, m1, m2, vs, vv, Cm.v0_for(m2), None, fields, spots, scales, sub)[0], one), sub


# ---- C. locate edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grid,cases", SC.LOCATE_EDGES, ids=[e[0].split(":")[0].replace(" ", "_") for e in SC.LOCATE_EDGES])
def test_locate_edges(emu, name, grid, cases):
    s = np.array([grid])
    m1, m2 = s.shape[1] - 1, 4
    vv = np.array([[0.0, 0.01, 0.04, 0.2, 1.0]])
    field = SC.synthetic_field(m1, m2, 1)[None]
    spots = np.array([[x for x, _ in cases]])
    scales = np.array([[(-1.5, 2.0, 0.75)[q % 3] for q in range(len(cases))]])
    out, flags = sample_field(emu, m1, m2, s, vv, 0.04, None, field, spots, scales, [1])
    row = field[0, 0, 2 * (m1 + 1):3 * (m1 + 1)]
    for q, (x, want) in enumerate(cases):
        if want[0] == "hit":
            assert flags[0, q] == 0 and out[0, 0, q] == row[want[1]] * scales[0, q], (name, x)
        elif want[0] == "interior":
            idx, w, flag = R.taps(s[0], x)
            assert flag == 0 and idx[0] == want[1]
            u = row[idx]
            ref = ((((w[0] * u[0]) + w[1] * u[1]) + w[2] * u[2]) + w[3] * u[3]) * scales[0, q]
            assert flags[0, q] == 0 and abs(out[0, 0, q] - ref) <= SC.TIGHT * np.abs(w * u).sum() * abs(scales[0, q]), (name, x, out[0, 0, q], ref)
        else:
            assert flags[0, q] == (R.OFF_GRID if want[0] == "off" else R.DEGENERATE) and math.isnan(out[0, 0, q]), (name, x, flags[0, q])
