"""Bermudan and knock-out barrier sweeps on the device over their admitted domain.  tests/test_gpu_bermudan.py and
tests/test_gpu_barrier.py run one case per kernel on a handful of grids whose m1 is even and whose barriers sit at fractions of
near-equal strikes; this file runs

  A. every row of event_cases.SHAPES on the streaming kernels (either side of every change of (B, G), of the chunk counts and of
     the sequential passes) and the LDS rows on the whole-loop kernels, barriers on event_cases.live_ranges;
  B. streams = 2 on small grids, so that the second sub-batch reads the dividend, exercise and monitoring tables at an offset,
     and the two Jacobian launchers with a group boundary inside a sub-batch;
  C. events on, before and after the paying steps of dividend schedules (event_cases.schedules_near_dividends);
  D. per-instance v-grids, models, step grids, schedules, barriers and rebates in one call on every kernel family, and the
     regimes R0, R6, T3, T5 (tests/regimes.py, tests/time_regimes.py) with events;
  E. profiling with events, and one handle alternating vanilla, Bermudan and barrier calls through the graph cache.

The reference is tests/bermudan_ref.py / tests/barrier_ref.py.  Bounds are the project's: field 1e-10 of the instance's max|U_ref|
(test_gpu_barrier.field_check, with its zero-field rule) on well-conditioned grids (asserted), prices 1e-9, J 2e-4.  Every case
pins its tuning keys, restores them, and asserts its kernel family from describe_last_sweep()."""
import functools
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import barrier_ref as KR
import bermudan_ref as BR
import common as Cm
import dividend_schedules as D
import event_cases as E
import regimes as R
import time_regimes as TR
from test_gpu_barrier import field_check, st, tuned

pytestmark = pytest.mark.gpu

BER, BAR = "bermudan", "barrier"
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
STREAM_KERNEL = {BER: "hadi_exercise_kernel after each of", BAR: "hadi_knockout_kernel after each of"}
LOOP_EVENT = {BER: "Bermudan: exercise at the end of", BAR: "barrier: knock-out at the end of"}
BLOCK8, BLOCK4 = {"small_seq": 0, "small_waves": 8}, {"small_seq": 0, "small_waves": 4}
SEQ, SEQ2 = {"small_seq": 1, "small_pairs": 0}, {"small_seq": 1, "small_pairs": 1}


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False, mixed=False):
    """(strikes, grids, payoff) on well-conditioned grids (asserted), built once per shape and left unchanged.  mixed: every
    instance on its own v-grid (Cm.mixed_vgrid_batch)."""
    if mixed:
        strikes, grids, _ = Cm.mixed_vgrid_batch(m1, m2, n)
    else:
        strikes = Cm.well_conditioned_strikes(m1, n)
        grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
        Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0


def _freeze(x):
    if x is None or isinstance(x, (int, float, str, bool)):
        return x
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return tuple(_freeze(y) for y in x)


class Ev:
    """One call with events: what (BER / BAR), the shape, the batch and everything that may differ per instance."""
    _REF = {}

    def __init__(self, what, m1, m2, n, N, events, put=False, dt=None, theta=Cm.THETA, rates=(Cm.R_D, Cm.R_F), models=None, mixed=False,
                 N_i=None, dt_i=None, bar=None, div=None, scheme=0):
        self.what, self.m1, self.m2, self.n, self.N, self.events, self.put = what, m1, m2, n, N, events, put
        self.dt = Cm.T / N if dt is None else dt
        self.theta, self.rates, self.models, self.mixed, self.N_i, self.dt_i, self.div, self.scheme = theta, rates, models, mixed, N_i, dt_i, div, scheme
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put, mixed)
        if what == BAR and bar is None:
            bar = E.barrier_batch(self.grids.Vec_s, self.strikes)[:3]
        self.bar = bar

    def head(self):
        return (self.m1, self.m2, self.N, self.dt, self.theta) + tuple(self.rates) + MODEL + (self.grids,)

    def kw(self):
        per = {}
        if self.models is not None:
            per.update(R.per_instance(self.models))
        if self.N_i is not None:
            per.update(N_i=list(self.N_i), delta_t_i=list(self.dt_i))
        k = dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*self.div) if self.div else None, scheme=self.scheme,
                 per_instance=per or None)
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        return k

    def run(self, sv, events=None):
        U = self.U0.copy()
        ev = self.events if events is None else events
        if self.what == BER:
            sv.bermudan_timestepping(*self.head(), U, ev, **self.kw())
        else:
            lo, up, reb = self.bar
            sv.barrier_timestepping(*self.head(), U, ev, lower=lo, upper=up, rebate=reb, **self.kw())
        return U, sv.describe_last_sweep()

    def vanilla(self, sv):
        U = self.U0.copy()
        sv.DO_timestepping(*self.head(), U, **self.kw())
        return U, sv.describe_last_sweep()

    def ref(self, events=None, rows=None):
        """Computed once per distinct input, shared by the cases that need it and left unchanged."""
        ev = self.events if events is None else events
        key = _freeze((self.what, self.m1, self.m2, self.n, self.N, self.dt, self.theta, self.rates, self.models, self.mixed, self.N_i,
                       self.dt_i, ev, self.put, self.div, self.bar, self.scheme, rows))
        if key not in self._REF:
            g = self.grids
            head = (self.m1, self.m2, self.N, self.dt, self.theta) + tuple(self.rates) + MODEL + (g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v,
                                                                                                  self.U0, ev)
            kw = dict(dividends=self.div, put_strikes=self.strikes if self.put else None, scheme=self.scheme, N_i=self.N_i, dt_i=self.dt_i,
                      models=self.models, rows=rows)
            U = BR.solve_batch(*head, **kw) if self.what == BER else KR.solve_batch(*head, *self.bar, **kw)
            U.setflags(write=False)
            self._REF[key] = U
        return self._REF[key]


def has(d, want, absent=()):
    for w in want:
        assert any(x in d for x in ((w,) if isinstance(w, str) else w)), (w, d)
    for a in absent:
        assert a not in d, (a, d)


def check(sv, name, case, tuning, want, absent=(), rows=None):
    with tuned(sv, tuning):
        U, d = case.run(sv)
    has(d, want, absent)
    field_check(name, U, case.ref(rows=rows), rows)
    return U, d


# ---- A. shapes ------------------------------------------------------------------------------------------------------------------
def streaming_rows():
    out = []
    for k, s in enumerate(E.SHAPES):
        for strip in ((0, 1) if 64 < s.m1 <= 1024 else (None,)):
            out.append((k, s, strip))
    return out


STREAM_IDS = ["%s-%dx%d-%s" % (s.name, s.m1, s.m2, {None: "plan", 0: "ring", 1: "strips"}[strip]) for _, s, strip in streaming_rows()]


def pass_kernels(m1, m2, strip):
    """What the description must name: the row pass of the shape's nodes-per-lane class and the column pass of its chunk count."""
    B, G = E.pick_shape(m1)
    if m1 > 1024:
        row = "hadi_pass_a_seq<EU>"
    elif strip:
        row = "hadi_pass_a_strip<8,EU,double,2>" if G == 2 else ("hadi_pass_a_strip<%d,EU>" % B, "hadi_pass_a_pairs<")
    else:
        row = "hadi_pass_a<%d,%d," % (B, G)
    P = (m2 + 1 + 32) // 33
    return [row, "hadi_pass_b_seq<EU>" if P > 16 else "(%d chunks of 33 rows" % P]


def small(m1, m2):
    """More instances and steps on the small shapes, the fewest on the large ones."""
    return (5, 3) if m1 <= 129 and m2 <= 66 else (3, 2)


@pytest.mark.parametrize("k,s,strip", streaming_rows(), ids=STREAM_IDS)
def test_streaming_shapes_barrier_on_the_live_ranges(solver, k, s, strip):
    n, N = small(s.m1, s.m2)
    strikes, grids, _ = batch(s.m1, s.m2, n)
    lo, up, reb, iab, names = E.barrier_batch(grids.Vec_s, strikes, E.turn(k))
    case = Ev(BAR, s.m1, s.m2, n, N, [1, N], bar=(lo, up, reb))
    tuning = st() if strip is None else st(strip=strip)
    U, _ = check(solver, "%s %s" % (s.name, names), case, tuning, pass_kernels(s.m1, s.m2, strip) + [STREAM_KERNEL[BAR] + " 2 monitoring steps"],
                 [LOOP_EVENT[BAR]])
    Ur = U.reshape(n, s.m2 + 1, s.m1 + 1)
    for i in range(n):  # monitored at N: exactly the nodes outside the table's range hold the rebate
        ia, ib = iab[i]
        assert (Ur[i][:, :ia] == reb[i]).all() and (Ur[i][:, ib + 1:] == reb[i]).all() and (Ur[i][:, ia:ib + 1] != reb[i]).any(), (i, names[i])


@pytest.mark.parametrize("k,s,strip", streaming_rows(), ids=STREAM_IDS)
def test_streaming_shapes_bermudan_put(solver, k, s, strip):
    n, N = small(s.m1, s.m2)
    tuning = st() if strip is None else st(strip=strip)
    check(solver, s.name, Ev(BER, s.m1, s.m2, n, N, [1, N], put=True), tuning,
          pass_kernels(s.m1, s.m2, strip) + [STREAM_KERNEL[BER] + " 2 exercise steps"], [LOOP_EVENT[BER]])


_LDS_MAX = {}


def largest_lds_m2(sv, m1):
    """The largest m2 at which the product's own route still takes a whole-loop LDS kernel on m1 s-intervals: found from
    describe_last_sweep() of one-step calls, with the next m2 asserted to stream."""
    if m1 not in _LDS_MAX:
        def lds(m2):  # (only the route is read: the grid of a scanned m2 need not be well-conditioned)
            strikes = Cm.well_conditioned_strikes(m1, 1)
            grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
            U = grids.call_payoff(strikes)
            sv.barrier_timestepping(m1, m2, 1, Cm.T, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, grids, U, [1], lower=0.7 * np.asarray(strikes))
            d = sv.describe_last_sweep()
            assert ("hadi_small_" in d) != ("row pass" in d), d
            return "hadi_small_" in d
        m2 = 20
        assert lds(m2)
        while lds(m2 + 1):
            m2 += 1
            assert m2 < 64
        _LDS_MAX[m1] = m2
    return _LDS_MAX[m1]


LDS_PATHS = [("block4", BLOCK4, "hadi_small_kernel<%d,4,EU>"), ("block8", BLOCK8, "hadi_small_kernel<%d,8,EU>"),
             ("seq", SEQ, "hadi_small_seq_kernel<%d>"), ("seq2", SEQ2, "hadi_small_seq2_kernel<%d>")]
LDS_IDS = ["%dx%d" % r for r in E.LDS_ROWS] + ["128xmax"]


def lds_shape(sv, row):
    return E.LDS_ROWS[row] if row < len(E.LDS_ROWS) else (128, largest_lds_m2(sv, 128))


@pytest.mark.parametrize("pname,tuning,kernel", LDS_PATHS, ids=[p[0] for p in LDS_PATHS])
@pytest.mark.parametrize("row", range(7), ids=LDS_IDS)
@pytest.mark.parametrize("what", [BER, BAR])
def test_lds_shapes(solver, what, row, pname, tuning, kernel):
    m1, m2 = lds_shape(solver, row)
    B = E.pick_shape(m1)[0]
    n, N = 5, 3
    if what == BAR:
        strikes, grids, _ = batch(m1, m2, n)
        case = Ev(BAR, m1, m2, n, N, [1, N], bar=E.barrier_batch(grids.Vec_s, strikes, row)[:3])
    else:
        case = Ev(BER, m1, m2, n, N, [1, N], put=True)
    if pname == "seq2" and m2 + 1 > 32:  # the pairs kernel holds at most 32 v-rows: small_pairs = 1 runs the one-instance kernel
        kernel, absent = "hadi_small_seq_kernel<%d>", ["seq2"]
    else:
        absent = []
    check(solver, "%s %dx%d" % (pname, m1, m2), case, tuning, [kernel % B, LOOP_EVENT[what] + " 2 steps"], absent + [STREAM_KERNEL[what]])


def test_two_nodes_per_lane_leave_the_lds_kernels_before_33_rows(solver):
    m1, m2 = E.NOT_LDS
    assert largest_lds_m2(solver, m1) < m2 == largest_lds_m2(solver, 64)
    with tuned(solver, SEQ2):
        _, d = Ev(BAR, m1, m2, 3, 2, [1, 2]).run(solver)
    has(d, ["row pass", STREAM_KERNEL[BAR]], ["hadi_small_"])


SCHEMES = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("row", range(7), ids=LDS_IDS)
@pytest.mark.parametrize("what", [BER, BAR])
def test_lds_shapes_scheme_kernel(solver, what, row, scheme, theta, sname):
    """Call data (the schemes' reference is the call's)."""
    m1, m2 = lds_shape(solver, row)
    n, N = 3, 3
    if what == BAR:
        strikes, grids, _ = batch(m1, m2, n)
        case = Ev(BAR, m1, m2, n, N, [1, N], bar=E.barrier_batch(grids.Vec_s, strikes, row + 3)[:3], scheme=scheme, theta=theta)
    else:
        case = Ev(BER, m1, m2, n, N, [1, N], scheme=scheme, theta=theta)
    check(solver, "sch %s %dx%d" % (sname, m1, m2), case, {"small_sch": 1},
          ["hadi_small_sch_kernel<%d,%s>" % (E.pick_shape(m1)[0], sname), LOOP_EVENT[what]], [STREAM_KERNEL[what]])


# ---- B. streams = 2 on small grids ----------------------------------------------------------------------------------------------
N5, T5 = [6, 4, 5, 3, 6], [1.0, 0.5, 0.8, 0.3, 0.7]
DT5 = [t / k for t, k in zip(T5, N5)]
EV5 = [[2, 6], [1, 3, 4], [], [3], [1, 2, 3, 4, 5, 6]]
DIV5 = ([0.2, 0.4, 0.6, 0.8], [0.5, 3.0, 0.2, 0.1], [0.02, 0.05, 0.02, 0.02])


@pytest.mark.parametrize("m1,m2", [(50, 25), (128, 64)], ids=["50x25", "128x64"])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
@pytest.mark.parametrize("what", [BER, BAR])
def test_two_streams_three_tables_three_offsets(solver, what, put, m1, m2):
    """Five instances in two sub-batches: the second reads the dividend table (per-instance dating: N_i, dt_i), the event table
    (per-instance schedules) and, for the barrier, the ranges and rebates from its own offset.  The rows of the tables differ
    between the halves (asserted), so a sub-batch that read from offset 0 would compute another instance's events."""
    n = 5
    flags = [D.flags(N5[k], DT5[k], DIV5[0], max(N5)) for k in range(n)]
    assert all(any(f >= 0 for f in row) for row in flags) and flags[0] != flags[3] and flags[1] != flags[4] and EV5[0] != EV5[3]
    case = Ev(what, m1, m2, n, max(N5), EV5, put=put, N_i=N5, dt_i=DT5, div=DIV5)
    with tuned(solver, st(streams=2)):
        U2, d2 = case.run(solver)
    with tuned(solver, st(streams=1)):
        U1, d1 = case.run(solver)
    has(d2, ["two streams", "sub-batches", STREAM_KERNEL[what]])
    has(d1, [STREAM_KERNEL[what]], ["two streams"])
    field_check("two streams %s %dx%d" % (what, m1, m2), U2, case.ref())
    assert np.array_equal(U1, U2)


@pytest.mark.parametrize("what", [BER, BAR])
def test_jacobian_launchers_with_a_group_boundary_inside_a_sub_batch(solver, what):
    """n0 = 3 on 128x64 with streams = 2: 18 instances in halves of 9, so the groups (base, kappa, eta, sigma, rho, V_0) of three
    change inside each half.  V_0_i, per-instance schedules, barriers and rebates."""
    m1, m2, n, N, eps = 128, 64, 3, 4, 1e-6
    strikes, grids, U0 = batch(m1, m2, n)
    ev = [[2, 4], [3], [1, 2, 4]]
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    head = (Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F) + MODEL + (m1, m2, size, N, Cm.THETA, Cm.T / N, n, grids)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, ev)
    refkw = dict(put_strikes=strikes, V_0_i=v0s)
    with tuned(solver, st(streams=2)):
        if what == BER:
            prices = solver.compute_base_prices_bermudan(*head, ws, ev, per_instance=per)
            J, base = solver.compute_jacobian_bermudan(*head, U0.copy(), ev, eps=eps, per_instance=per)
        else:
            lo, up, reb = E.barrier_batch(grids.Vec_s, strikes, 4)[:3]
            refkw.update(lower=lo, upper=up, rebate=reb)
            prices = solver.compute_base_prices_barrier(*head, ws, ev, lower=lo, upper=up, rebate=reb, per_instance=per)
            J, base = solver.compute_jacobian_barrier(*head, U0.copy(), ev, lower=lo, upper=up, rebate=reb, eps=eps, per_instance=per)
        d = solver.describe_last_sweep()
    has(d, ["two streams", "2 sub-batches of 9 instances", STREAM_KERNEL[what]])
    ref = BR if what == BER else KR
    Jo, bo = ref.jacobian(*args, eps=eps, **refkw)
    print("launchers %s: prices %.2e, J %.2e" % (what, np.abs(base - bo).max(), np.abs(J - Jo).max()))
    assert np.abs(prices - bo).max() <= 1e-9 and np.abs(base - bo).max() <= 1e-9
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


# ---- C. events next to dividends ------------------------------------------------------------------------------------------------
NEAR = E.schedules_near_dividends(20, Cm.T / 20, Cm.T)[:3] + E.schedules_near_dividends(10, Cm.T / 10, Cm.T)[-6:]
NEAR_PUT = [(c, p) for c in NEAR for p in (False, True) if (c.puts if p else c.calls)]
NEAR_IDS = ["%s-%s" % (c.name.replace(" ", "_"), "put" if p else "call") for c, p in NEAR_PUT]
LOF, UPF = (0.7, 0.8, 0.6), (1.3, 1.2, 1.4)
PATHS_50 = [("block4", BLOCK4, "hadi_small_kernel<1,4,EU>"), ("block8", BLOCK8, "hadi_small_kernel<1,8,EU>"),
            ("seq", SEQ, "hadi_small_seq_kernel<1>"), ("seq2", SEQ2, "hadi_small_seq2_kernel<1>"), ("ring", st(), "hadi_pass_a<1,1,")]


def near_case(what, m1, m2, case, put):
    n = 3
    strikes, grids, _ = batch(m1, m2, n, put)
    for k in range(n):
        E.check(case, grids.Vec_s[k])
    if case.barrier == "floor":  # nodes 0 .. 2 knocked, rebate 2: the jump's node-0 reads meet the rebate, its nonpos branch returns 0
        bar = E.floor_barrier(grids.Vec_s) + (np.full(n, 2.0),)
    else:
        bar = (np.array(LOF) * strikes, np.array(UPF) * strikes, np.array(E.REBATES[:n]))
    return Ev(what, m1, m2, n, case.N, case.events, put=put, dt=case.dt, div=case.dividends, bar=bar if what == BAR else None)


def test_the_near_cases_are_the_ones_named():
    assert [c.name for c in NEAR] == ["before the paying steps", "on the paying steps", "every step", "step1", "lastN", "alternate",
                                      "big_cash", "negative", "zero"]
    assert NEAR[0].events == [3, 7, 10, 15] and NEAR[1].events == [4, 8, 11, 16] and NEAR[2].events == list(range(1, 21))
    for what in (BER, BAR):  # the order of event and jump matters to the reference: condition on the reference alone
        for put in (False, True):
            a, b = near_case(what, 50, 25, NEAR[0], put).ref(), near_case(what, 50, 25, NEAR[1], put).ref()
            assert np.abs(a - b).max() / np.abs(a).max() >= 1e-4, (what, put)


@pytest.mark.parametrize("case,put", NEAR_PUT, ids=NEAR_IDS)
@pytest.mark.parametrize("what", [BER, BAR])
def test_events_next_to_dividends_50x25(solver, what, case, put):
    c = near_case(what, 50, 25, case, put)
    for pname, tuning, kernel in PATHS_50:
        loop = "hadi_small" in kernel
        check(solver, "%s %s" % (case.name, pname), c, tuning, [kernel, (LOOP_EVENT if loop else STREAM_KERNEL)[what]],
              [(STREAM_KERNEL if loop else LOOP_EVENT)[what]])


@pytest.mark.parametrize("case,put", NEAR_PUT, ids=NEAR_IDS)
@pytest.mark.parametrize("what", [BER, BAR])
def test_events_next_to_dividends_strips(solver, what, case, put):
    check(solver, "%s strips" % case.name, near_case(what, 300, 80, case, put), st(strip=1), ["hadi_pass_a_strip<8,", STREAM_KERNEL[what]],
          [LOOP_EVENT[what]])


# ---- D. per-instance everything -------------------------------------------------------------------------------------------------
#            name            m1    m2   n  tuning          kernel
FAMILIES = [("block8",       50,   25,  3, BLOCK8,         "hadi_small_kernel<1,8,EU>"),
            ("seq",          50,   25,  3, SEQ,            "hadi_small_seq_kernel<1>"),
            ("seq2",         50,   25,  5, SEQ2,           "hadi_small_seq2_kernel<1>"),
            ("sch_MCS",      50,   25,  3, {"small_sch": 1}, "hadi_small_sch_kernel<1,MCS>"),
            ("ring_b1",      50,   25,  3, st(),           "hadi_pass_a<1,1,"),
            ("ring_b2",      100,  50,  3, st(strip=0),    "hadi_pass_a<2,1,"),
            ("strips_b8",    300,  80,  3, st(strip=1),    "hadi_pass_a_strip<8,EU>"),
            ("paired_strips", 600, 30,  3, st(strip=1),    "hadi_pass_a_strip<8,EU,double,2>"),
            ("pass_a_seq",   1100, 30,  3, st(),           "hadi_pass_a_seq<EU>"),
            ("pass_b_seq",   40,   600, 3, st(),           "hadi_pass_b_seq<EU>")]
STEP_GRIDS = [(4, Cm.T / 4), (3, 0.5 / 3), (2, 0.25 / 2), (4, 0.8 / 4), (3, 0.6 / 3)]
EVENTS_I = [[1, 4], [2], [1, 2], [], [3]]


@pytest.mark.parametrize("name,m1,m2,n,tuning,kernel", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("what", [BER, BAR])
def test_per_instance_everything(solver, what, name, m1, m2, n, tuning, kernel):
    """Every instance on its own v-grid, model (neighbours never share one), step grid, schedule, barrier and rebate."""
    sch = name == "sch_MCS"
    models = R.rotating_models(n, 1)
    N_i, dt_i = [g[0] for g in STEP_GRIDS[:n]], [g[1] for g in STEP_GRIDS[:n]]
    bar = None
    if what == BAR:
        strikes, grids, _ = batch(m1, m2, n, not sch)
        bar = E.barrier_batch(grids.Vec_s, strikes, 4)[:3]
    case = Ev(what, m1, m2, n, max(N_i), EVENTS_I[:n], put=not sch, rates=R.MODEL_RATES, models=models, mixed=True, N_i=N_i, dt_i=dt_i,
              bar=bar, scheme=H.SCHEME_MCS if sch else 0, theta=TH_MCS if sch else Cm.THETA)
    assert len({g.tobytes() for g in case.grids.Vec_v}) >= 3 and all(models[k] != models[k + 1] for k in range(n - 1))
    loop = "hadi_small" in kernel
    check(solver, "per-instance %s %s" % (what, name), case, tuning, [kernel, (LOOP_EVENT if loop else STREAM_KERNEL)[what]],
          [(STREAM_KERNEL if loop else LOOP_EVENT)[what]])


REGIME_ROWS = [("ring_b1", 50, 25, st(), "hadi_pass_a<1,1,", "hadi_pass_a<1,1,"),
               ("strips_b8", 300, 80, st(strip=1), "hadi_pass_a_strip<8,EU>", "hadi_pass_a<8,1,"),
               ("seq", 50, 25, SEQ, "hadi_small_seq_kernel<1>", "hadi_small_seq_kernel<1>")]
REGIMES = ["R0", "R6", "T3", "T5"]


@pytest.mark.parametrize("rid", REGIMES)
@pytest.mark.parametrize("name,m1,m2,tuning,kernel,ring", REGIME_ROWS, ids=[r[0] for r in REGIME_ROWS])
@pytest.mark.parametrize("what", [BER, BAR])
def test_regimes_with_events(solver, what, name, m1, m2, tuning, kernel, ring, rid):
    """R0 (q = 0) and T3 (theta = 0) switch the strips off: those rows must describe the shared ring.  Each regime's reference
    differs from the canonical one (same events) by >= 1e-6 of max|U|, so a kernel on the wrong rate, theta or dt cannot pass."""
    n, N0 = 3, 3
    if rid in R.RATE:
        rates, (theta, dt, N) = R.RATE[rid], TR.canonical(N0)
        canon = dict(rates=R.CANONICAL_RATES, theta=theta, dt=dt)
    else:
        rates, (theta, dt, N) = R.CANONICAL_RATES, TR.regime(rid, N0)
        canon = dict(rates=rates, theta=TR.canonical(N)[0], dt=TR.canonical(N)[1])
    events = [1] if N == 1 else [1, N]
    off = rid in R.Q_ZERO or rid in TR.EXPLICIT
    case = Ev(what, m1, m2, n, N, events, put=True, rates=rates, theta=theta, dt=dt)
    twin = Ev(what, m1, m2, n, N, events, put=True, bar=case.bar, **canon)
    Uo, Uc = case.ref(), twin.ref()
    moved = np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)
    assert moved.min() >= 1e-6, moved
    loop = "hadi_small" in kernel
    check(solver, "%s %s %s" % (rid, what, name), case, tuning, [ring if off else kernel, (LOOP_EVENT if loop else STREAM_KERNEL)[what]],
          ["strip"] if off else [])


# ---- E. profiling and the graph cache -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [BER, BAR])
def test_profiling_with_events(solver, what):
    """Profiling sends the call to the streaming kernels, with the event kernel behind the listed steps."""
    N = 6
    case = Ev(what, 50, 25, 3, N, [2, 6], put=True)
    with tuned(solver, st()):
        plain, _ = case.run(solver)
    solver.set_profiling(True)
    try:
        U, d = case.run(solver)  # (default tuning: without profiling this batch runs a whole-loop LDS kernel)
        t = solver.timing()
    finally:
        solver.set_profiling(False)
    has(d, ["hadi_pass_a<1,1,", "hadi_pass_b<", STREAM_KERNEL[what]], ["hadi_small_"])
    assert t["pass_a_launches"] == N and t["pass_b_launches"] == N, t
    assert np.array_equal(U, plain)
    field_check("profiling " + what, U, case.ref())
    _, d0 = case.run(solver)
    has(d0, ["hadi_small_", LOOP_EVENT[what]])


def test_graph_cache_vanilla_bermudan_barrier_alternating(solver):
    """One handle, one shape, one N: vanilla, Bermudan, barrier, and again -- three captures, three replays, every result its own
    kind's and each replay bit for bit its first run."""
    N, ev = 7, [2, 6]
    ber, bar = Ev(BER, 50, 25, 3, N, ev, put=True), Ev(BAR, 50, 25, 3, N, ev, put=True)
    Uv = np.stack([BR.solve_batch(*ber.head()[:-1], ber.grids.Vec_s, ber.grids.Vec_v, ber.grids.Delta_s, ber.grids.Delta_v, ber.U0, [],
                                  put_strikes=ber.strikes)])[0]
    Ub, Uk = ber.ref(), bar.ref()
    for a, b in ((Uv, Ub), (Uv, Uk), (Ub, Uk)):
        assert np.abs(a - b).max() / np.abs(a).max() >= 1e-4
    with tuned(solver, st(graph=1)):
        # (the buffers each kind needs are grown first -- growing one would empty the cache -- by calls with other keys)
        Ev(BER, 50, 25, 3, N + 2, [1], put=True).vanilla(solver)
        ber.run(solver, events=[1, 5])
        bar.run(solver, events=[1, 5])
        c0 = Cm.graph_counts(solver)
        got = [ber.vanilla(solver), ber.run(solver), bar.run(solver), ber.vanilla(solver), ber.run(solver), bar.run(solver)]
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert (delta["captures"], delta["replays"]) == (3, 3), delta
    for k, (U, d) in enumerate(got):
        has(d, ["hadi_pass_a<1,1,"] + ([STREAM_KERNEL[BER]] if k % 3 == 1 else [STREAM_KERNEL[BAR]] if k % 3 == 2 else []),
            ["Bermudan", "barrier"] if k % 3 == 0 else [])
        field_check("graph call %d" % k, U, (Uv, Ub, Uk)[k % 3])
    for k in range(3):
        assert np.array_equal(got[k][0], got[k + 3][0])
