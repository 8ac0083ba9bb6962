"""Forward-start and cliquet sweeps on the device over their admitted domain.  tests/test_gpu_cliquet.py runs one case per kernel
on a handful of grids whose m1 is even; this file runs

  A. every row of event_cases.SHAPES on the streaming kernels (either side of every change of (B, G), of the chunk counts and of
     the sequential passes) followed by hadi_fixing_gather_kernel and hadi_fixing_kernel, and the LDS rows on the whole-loop
     kernels (hadi_fixing_lds): the reference nodes on the placements of fixing_cases.reference_nodes, put data, every instance
     with its own row of weights (zero and non-zero at N);
  B. streams = 2 on small grids, so that the second sub-batch reads the fixing table, the weights, the located nodes, the modes,
     c and the s-grids at an offset -- with per-instance rows and with one shared row (table stride 0) -- and the two Jacobian
     launchers with a group boundary inside a sub-batch;
  C. fixings on, before and after the paying steps of dividend schedules (fixing_cases.near_fixings);
  D. per-instance v-grids, models, step grids, schedules, reference nodes, modes and weights in one call on every kernel family,
     and the regimes R0, R6, T3, T5 (tests/regimes.py, tests/time_regimes.py) with fixings;
  E. profiling with fixings, and one handle alternating vanilla, Bermudan, barrier and cliquet calls through the graph cache.

The reference is tests/cliquet_ref.py.  Bounds are those of tests/test_gpu_cliquet.py: field 1e-10 of the instance's max|U_ref|
on well-conditioned grids (asserted), prices 1e-9, J 2e-4.  That field bound has no rule for a zero field, so every case here
asserts max|U_ref| >= 1e-3 for every instance (put data wherever a RETURN fixing may sit at node 0, where call data give
max|U| ~ 1e-16); tests/test_emu_fixing_domain.py shows on the CPU that a reference node off by one moves every instance of the
shape batches by >= 1e-4 of max|U_ref|.  Every case pins its tuning keys, restores them, and asserts its kernel family from
describe_last_sweep()."""
import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import bermudan_ref as BR
import cliquet_ref as QR
import common as Cm
import dividend_schedules as D
import event_cases as E
import fixing_cases as F
import regimes as R
import test_gpu_event_domain as ED
import time_regimes as TR
from test_gpu_cliquet import FIX_LOOP, FIX_STREAM, field_check, st, tuned

pytestmark = pytest.mark.gpu

MODEL = F.MODEL
SHARES, RETURN = H.FIX_SHARES, H.FIX_RETURN
assert (SHARES, RETURN) == (F.SHARES, F.RETURN)
has, batch = ED.has, ED.batch


class Fx:
    """One call with fixings: the shape, the batch and everything that may differ per instance.  turn: the placements of
    fixing_cases.fixing_batch; None: reference nodes around the strikes (fixing_cases.strike_batch)."""

    def __init__(self, m1, m2, n, N, fix, weights, turn=None, put=True, dt=None, theta=Cm.THETA, rates=(Cm.R_D, Cm.R_F), models=None,
                 mixed=False, N_i=None, dt_i=None, div=None, scheme=0, place=None):
        self.m1, self.m2, self.n, self.N, self.fix, self.weights, self.put = m1, m2, n, N, fix, weights, put
        self.dt = Cm.T / N if dt is None else dt
        self.theta, self.rates, self.models, self.mixed, self.N_i, self.dt_i, self.div, self.scheme = theta, rates, models, mixed, N_i, dt_i, div, scheme
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put, mixed)
        vs = self.grids.Vec_s
        if place is not None:
            self.ref_spot, self.mode, self.i_ref = place
            self.names = ["given"] * n
        elif turn is None:
            self.ref_spot, self.mode, self.i_ref = F.strike_batch(vs, self.strikes)
            self.names = ["near the strike"] * n
        else:
            self.ref_spot, self.mode, self.i_ref, self.names = F.fixing_batch(vs, turn)

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

    def run(self, sv, fix=None, weights="own"):
        U = self.U0.copy()
        sv.cliquet_timestepping(*self.head(), U, self.fix if fix is None else fix, self.ref_spot, self.mode,
                                self.weights if isinstance(weights, str) else weights, **self.kw())
        return U, sv.describe_last_sweep()

    def ref(self, rows=None):
        g = self.grids
        return F.reference(self.m1, self.m2, self.N, self.dt, self.theta, tuple(self.rates), (g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v), self.U0,
                           self.fix, self.ref_spot, self.mode, self.weights, self.strikes, self.put, self.div, self.scheme, self.N_i, self.dt_i,
                           self.models, rows)


def checked(name, U, Uo):
    """field_check, never against a zero field."""
    scale = np.abs(Uo).max(axis=1)
    assert (scale >= 1e-3).all(), (name, scale)
    field_check(name, U, Uo)


def check(sv, name, case, tuning, want, absent=()):
    with tuned(sv, tuning):
        U, d = case.run(sv)
    has(d, want, absent)
    checked(name, U, case.ref())
    return U, d


def shape_case(m1, m2, n, N, turn, **kw):
    fix, w = F.shape_schedule(n, N)
    return Fx(m1, m2, n, N, fix, w, turn=turn, **kw)


def exact_bits(sv, case, tuning, U):
    """Where the fixing at N has weight 0: against the run whose schedules stop short of N, SHARES keeps the bits of column i_ref
    and RETURN makes every node of row j equal c_j's bits."""
    zero = [k for k in range(case.n) if case.weights[k][-1] == 0.0]
    assert zero and all(r[-1] == case.N for r in case.fix)
    with tuned(sv, tuning):
        V, _ = case.run(sv, fix=[r[:-1] for r in case.fix], weights=[r[:-1] for r in case.weights])
    Ur, Vr = U.reshape(case.n, case.m2 + 1, case.m1 + 1), V.reshape(case.n, case.m2 + 1, case.m1 + 1)
    for k in zero:
        c = Vr[k][:, case.i_ref[k]]
        assert np.array_equal(Ur[k][:, case.i_ref[k]].view(np.uint64), c.view(np.uint64)), (case.names[k], "column i_ref")
        if case.mode[k] == RETURN:
            flat = np.repeat(c[:, None], case.m1 + 1, axis=1)
            assert np.array_equal(Ur[k].view(np.uint64), flat.view(np.uint64)), (case.names[k], np.nonzero((Ur[k] != flat).any(axis=0))[0])


# ---- A. shapes ------------------------------------------------------------------------------------------------------------------
RUNS = F.streaming_runs()


def test_the_streaming_runs_are_the_rows_of_the_event_domain_tests():
    assert [r[0] for r in RUNS if "turn" not in r[0]] == ED.STREAM_IDS
    assert [(r[1], r[3]) for r in RUNS if "turn" not in r[0]] == [(k, strip) for k, _, strip in ED.streaming_rows()]


@pytest.mark.parametrize("sid,k,s,strip,turn", RUNS, ids=[r[0] for r in RUNS])
def test_streaming_shapes(solver, sid, k, s, strip, turn):
    n, N = ED.small(s.m1, s.m2)
    case = shape_case(s.m1, s.m2, n, N, turn)
    tuning = st() if strip is None else st(strip=strip)
    U, _ = check(solver, "%s %s" % (s.name, case.names), case, tuning, ED.pass_kernels(s.m1, s.m2, strip) + [FIX_STREAM + " 2 fixing steps"],
                 [FIX_LOOP])
    exact_bits(solver, case, tuning, U)


@pytest.mark.parametrize("pname,tuning,kernel", ED.LDS_PATHS, ids=[p[0] for p in ED.LDS_PATHS])
@pytest.mark.parametrize("row", range(7), ids=ED.LDS_IDS)
def test_lds_shapes(solver, row, pname, tuning, kernel):
    m1, m2 = ED.lds_shape(solver, row)
    B = E.pick_shape(m1)[0]
    case = shape_case(m1, m2, 5, 3, row)
    if pname == "seq2" and m2 + 1 > 32:  # the pairs kernel holds at most 32 v-rows: small_pairs = 1 runs the one-instance kernel
        kernel, absent = "hadi_small_seq_kernel<%d>", ["seq2"]
    else:
        absent = []
    U, _ = check(solver, "%s %dx%d %s" % (pname, m1, m2, case.names), case, tuning, [kernel % B, FIX_LOOP + " 2 steps"], absent + [FIX_STREAM])
    exact_bits(solver, case, tuning, U)


@pytest.mark.parametrize("scheme,theta,sname", ED.SCHEMES, ids=[s[2] for s in ED.SCHEMES])
@pytest.mark.parametrize("row", range(7), ids=ED.LDS_IDS)
def test_lds_shapes_scheme_kernel(solver, row, scheme, theta, sname):
    """Call data (the schemes' reference is the call's): the batch starts one placement on, so that no instance is RETURN at node
    0, where call data give a zero field."""
    m1, m2 = ED.lds_shape(solver, row)
    case = shape_case(m1, m2, 3, 3, 1, put=False, scheme=scheme, theta=theta)
    assert 0 not in case.i_ref
    check(solver, "sch %s %dx%d" % (sname, m1, m2), case, {"small_sch": 1},
          ["hadi_small_sch_kernel<%d,%s>" % (E.pick_shape(m1)[0], sname), FIX_LOOP], [FIX_STREAM])


def test_two_nodes_per_lane_leave_the_lds_kernels_before_33_rows(solver):
    m1, m2 = E.NOT_LDS
    assert ED.largest_lds_m2(solver, m1) < m2 == ED.largest_lds_m2(solver, 64)
    with tuned(solver, ED.SEQ2):
        _, d = shape_case(m1, m2, 3, 2, 0).run(solver)
    has(d, ["row pass", FIX_STREAM], ["hadi_small_"])


# ---- B. streams = 2 on small grids ----------------------------------------------------------------------------------------------
FIX5 = ED.EV5  # [[2, 6], [1, 3, 4], [], [3], [1, 2, 3, 4, 5, 6]] on the step grids N5, DT5


@pytest.mark.parametrize("m1,m2", [(50, 25), (128, 64)], ids=["50x25", "128x64"])
def test_two_streams_per_instance_rows(solver, m1, m2):
    """Five instances in two sub-batches: the second reads the dividend table (per-instance dating: N_i, dt_i), the fixing table and
    the weights (per-instance rows), the located nodes, the modes, c and the s-grids from its own offset.  The rows of the tables
    differ between the halves (asserted), so a sub-batch that read from offset 0 would compute another instance's event."""
    n = 5
    flags = [D.flags(ED.N5[k], ED.DT5[k], ED.DIV5[0], max(ED.N5)) for k in range(n)]
    w = F.mixed_weights(FIX5)
    case = Fx(m1, m2, n, max(ED.N5), FIX5, w, turn=2, N_i=ED.N5, dt_i=ED.DT5, div=ED.DIV5)
    assert all(any(f >= 0 for f in row) for row in flags) and flags[0] != flags[3] and flags[1] != flags[4]
    assert FIX5[0] != FIX5[3] and FIX5[1] != FIX5[4] and w[0] != w[3] and w[1] != w[4]
    assert case.i_ref[0] != case.i_ref[3] and case.i_ref[1] != case.i_ref[4] and case.mode[0] != case.mode[3]
    with tuned(solver, st(streams=2)):
        U2, d2 = case.run(solver)
    with tuned(solver, st(streams=1)):
        U1, d1 = case.run(solver)
    has(d2, ["two streams", "sub-batches", FIX_STREAM])
    has(d1, [FIX_STREAM], ["two streams"])
    checked("two streams, per-instance rows %dx%d" % (m1, m2), U2, case.ref())
    assert np.array_equal(U1, U2)


@pytest.mark.parametrize("m1,m2", [(50, 25), (128, 64)], ids=["50x25", "128x64"])
def test_two_streams_shared_row(solver, m1, m2):
    """One schedule and one weight list for the batch: the tables have one row and stride 0, so the second sub-batch must NOT
    offset them -- while it does offset the located nodes, the modes, c and the s-grids."""
    n, N = 5, 4
    fix = [1, 3, 4]
    case = Fx(m1, m2, n, N, fix, F.mixed_weights(fix), turn=2)
    assert F.mixed_weights(fix) == [1.0, 0.5, 0.0] and len(set(case.i_ref)) == 5
    with tuned(solver, st(streams=2)):
        U2, d2 = case.run(solver)
    with tuned(solver, st(streams=1)):
        U1, d1 = case.run(solver)
    has(d2, ["two streams", "sub-batches", FIX_STREAM + " 3 fixing steps"])
    has(d1, [FIX_STREAM], ["two streams"])
    checked("two streams, shared row %dx%d" % (m1, m2), U2, case.ref())
    assert np.array_equal(U1, U2)


def test_jacobian_launchers_with_a_group_boundary_inside_a_sub_batch(solver):
    """n0 = 3 on 128x64 with streams = 2: 18 instances in halves of 9, so the groups (base, kappa, eta, sigma, rho, V_0) of three
    change inside each half and the instances' rows wrap by k % 3.  V_0_i, per-instance schedules, reference nodes, modes and
    weights; the price is read at S_0, where instance 0 fixes."""
    m1, m2, n, N, eps = 128, 64, 3, 4, 1e-6
    strikes, grids, U0 = batch(m1, m2, n, True)
    fix = [[2, 4], [3], [1, 2, 4]]
    wts = [[1.0, 0.0], [0.5], [0.0, 0.25, 1.0]]
    vs = grids.Vec_s
    # (nodes around the strikes: the prices are held to an absolute bound, so none may be a zero price -- asserted below)
    i_ref = [QR.find_node(vs[0], Cm.S_0), int(np.argmin(np.abs(vs[1] - strikes[1]))) + 3, int(np.argmin(np.abs(vs[2] - strikes[2]))) - 2]
    assert i_ref[0] > 0 and len(set(i_ref)) == 3
    ref = np.array([vs[k][i_ref[k]] for k in range(n)])
    mode = [SHARES, RETURN, SHARES]
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    head = (Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F) + MODEL + (m1, m2, size, N, Cm.THETA, Cm.T / N, n, grids)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, fix)
    refkw = dict(put_strikes=strikes, V_0_i=v0s, ref_spot=ref, mode=np.asarray(mode), weights=wts)
    with tuned(solver, st(streams=2)):
        prices = solver.compute_base_prices_cliquet(*head, ws, fix, ref, mode, wts, per_instance=per)
        has(solver.describe_last_sweep(), [FIX_STREAM])
        J, base = solver.compute_jacobian_cliquet(*head, U0.copy(), fix, ref, mode, wts, eps=eps, per_instance=per)
        d = solver.describe_last_sweep()
    has(d, ["two streams", "2 sub-batches of 9 instances", FIX_STREAM])
    Jo, bo = QR.jacobian(*args, eps=eps, **refkw)
    print("launchers: prices %.2e, J %.2e" % (np.abs(base - bo).max(), np.abs(J - Jo).max()))
    assert np.abs(bo).min() >= 1e-3
    assert np.abs(prices - bo).max() <= 1e-9 and np.abs(base - bo).max() <= 1e-9
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


# ---- C. fixings next to dividends -----------------------------------------------------------------------------------------------
NEAR, NEAR_PUT, NEAR_IDS = ED.NEAR, ED.NEAR_PUT, ED.NEAR_IDS


def near_case(m1, m2, case, put):
    strikes, grids, _ = batch(m1, m2, 3, put)
    for k in range(3):
        E.check(case, grids.Vec_s[k])
    fix, w, ref, mode, i_ref = F.near_fixings(case, grids.Vec_s, strikes)
    return Fx(m1, m2, 3, case.N, fix, w, put=put, dt=case.dt, div=case.dividends, place=(ref, mode, i_ref))


def test_the_near_cases_are_the_ones_named():
    assert [c.name for c in NEAR] == ["before the paying steps", "on the paying steps", "every step", "step1", "lastN", "alternate",
                                      "big_cash", "negative", "zero"]
    assert NEAR[0].events == [3, 7, 10, 15] and NEAR[1].events == [4, 8, 11, 16] and NEAR[2].events == list(range(1, 21))
    for c in NEAR[-3:]:
        fx = near_case(50, 25, c, c.puts)
        assert c.barrier == "floor" and fx.i_ref[:2] == [0, 1] and fx.mode[:2] == [RETURN, SHARES]
    for put in (False, True):  # the order of fixing and jump matters to the reference: condition on the reference alone
        a, b = near_case(50, 25, NEAR[0], put).ref(), near_case(50, 25, NEAR[1], put).ref()
        assert np.abs(a - b).max() / np.abs(a).max() >= 1e-4, put


@pytest.mark.parametrize("case,put", NEAR_PUT, ids=NEAR_IDS)
def test_fixings_next_to_dividends_50x25(solver, case, put):
    c = near_case(50, 25, case, put)
    for pname, tuning, kernel in ED.PATHS_50:
        loop = "hadi_small" in kernel
        check(solver, "%s %s" % (case.name, pname), c, tuning, [kernel, FIX_LOOP if loop else FIX_STREAM], [FIX_STREAM if loop else FIX_LOOP])


@pytest.mark.parametrize("case,put", NEAR_PUT, ids=NEAR_IDS)
def test_fixings_next_to_dividends_strips(solver, case, put):
    check(solver, "%s strips" % case.name, near_case(300, 80, case, put), st(strip=1), ["hadi_pass_a_strip<8,", FIX_STREAM], [FIX_LOOP])


# ---- D. per-instance everything -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m1,m2,n,tuning,kernel", ED.FAMILIES, ids=[f[0] for f in ED.FAMILIES])
def test_per_instance_everything(solver, name, m1, m2, n, tuning, kernel):
    """Every instance on its own v-grid, model (neighbours never share one), step grid, schedule, reference node, mode and weights."""
    sch = name == "sch_MCS"
    models = R.rotating_models(n, 1)
    N_i, dt_i = [g[0] for g in ED.STEP_GRIDS[:n]], [g[1] for g in ED.STEP_GRIDS[:n]]
    fix = ED.EVENTS_I[:n]
    # (call data under the scheme kernel, whose reference is the call's; no placement of either batch is node 0)
    case = Fx(m1, m2, n, max(N_i), fix, F.mixed_weights(fix), turn=1 if sch else 2, put=not sch, rates=R.MODEL_RATES, models=models, mixed=True,
              N_i=N_i, dt_i=dt_i, scheme=H.SCHEME_MCS if sch else 0, theta=ED.TH_MCS if sch else Cm.THETA)
    assert len({g.tobytes() for g in case.grids.Vec_v}) >= 3 and all(models[k] != models[k + 1] for k in range(n - 1))
    assert len(set(case.i_ref)) == n and len(set(case.mode)) == 2
    loop = "hadi_small" in kernel
    check(solver, "per-instance %s" % name, case, tuning, [kernel, FIX_LOOP if loop else FIX_STREAM], [FIX_STREAM if loop else FIX_LOOP])


@pytest.mark.parametrize("rid", F.REGIMES)
@pytest.mark.parametrize("name,m1,m2,tuning,kernel,ring", ED.REGIME_ROWS, ids=[r[0] for r in ED.REGIME_ROWS])
def test_regimes_with_fixings(solver, name, m1, m2, tuning, kernel, ring, rid):
    """R0 (q = 0) and T3 (theta = 0) switch the strips off: those rows must describe the shared ring.  Each regime's reference
    differs from the canonical one (same fixings) by >= 1e-6 of max|U|, so a kernel on the wrong rate, theta or dt cannot pass."""
    assert (m1, m2) in F.REGIME_SHAPES
    rates, theta, dt, N, fix, canon = F.regime_inputs(rid)
    off = rid in R.Q_ZERO or rid in TR.EXPLICIT
    w = F.mixed_weights(fix)
    case = Fx(m1, m2, 3, N, fix, w, rates=rates, theta=theta, dt=dt)
    twin = Fx(m1, m2, 3, N, fix, w, **canon)
    Uo, Uc = case.ref(), twin.ref()
    moved = np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)
    assert moved.min() >= 1e-6, moved
    loop = "hadi_small" in kernel
    check(solver, "%s %s" % (rid, name), case, tuning, [ring if off else kernel, FIX_LOOP if loop else FIX_STREAM], ["strip"] if off else [])


# ---- E. profiling and the graph cache -------------------------------------------------------------------------------------------
def test_profiling_with_fixings(solver):
    """Profiling sends the call to the streaming kernels, with the two fixing kernels behind the listed steps."""
    N = 6
    fix = [2, 6]
    case = Fx(50, 25, 3, N, fix, F.mixed_weights(fix), turn=0)
    with tuned(solver, st()):
        plain, _ = case.run(solver)
    solver.set_profiling(True)
    try:
        U, d = case.run(solver)  # (default tuning: without profiling this batch runs a whole-loop LDS kernel)
        t = solver.timing()
    finally:
        solver.set_profiling(False)
    has(d, ["hadi_pass_a<1,1,", "hadi_pass_b<", FIX_STREAM], ["hadi_small_"])
    assert t["pass_a_launches"] == N and t["pass_b_launches"] == N, t
    assert np.array_equal(U, plain)
    checked("profiling", U, case.ref())
    _, d0 = case.run(solver)
    has(d0, ["hadi_small_", FIX_LOOP])


def test_graph_cache_vanilla_bermudan_barrier_cliquet_alternating(solver):
    """One handle, one shape, one N: vanilla, Bermudan, barrier, cliquet, and again -- four captures, four replays, every result its
    own kind's and each replay bit for bit its first run.  (Thirteen steps: no other test of the session captures these loops.)"""
    N, ev = 13, [3, 9]
    ber, bar = ED.Ev(ED.BER, 50, 25, 3, N, ev, put=True), ED.Ev(ED.BAR, 50, 25, 3, N, ev, put=True)
    fx = Fx(50, 25, 3, N, ev, F.mixed_weights(ev))
    g = ber.grids
    Uv = BR.solve_batch(*ber.head()[:-1], g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, ber.U0, [], put_strikes=ber.strikes)
    refs = (Uv, ber.ref(), bar.ref(), fx.ref())
    for a in range(4):
        for b in range(a + 1, 4):
            assert np.abs(refs[a] - refs[b]).max() / np.abs(refs[a]).max() >= 1e-4, (a, b)
    with tuned(solver, st(graph=1)):
        # (the buffers each kind needs are grown first -- growing one would empty the cache -- by calls with other keys)
        ED.Ev(ED.BER, 50, 25, 3, N + 2, [1], put=True).vanilla(solver)
        ber.run(solver, events=[1, 5])
        bar.run(solver, events=[1, 5])
        fx.run(solver, fix=[1, 5])
        c0 = Cm.graph_counts(solver)
        calls = (ber.vanilla, ber.run, bar.run, fx.run)
        got = [f(solver) for f in calls + calls]
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert (delta["captures"], delta["replays"]) == (4, 4), delta
    marks = ([], [ED.STREAM_KERNEL[ED.BER]], [ED.STREAM_KERNEL[ED.BAR]], [FIX_STREAM])
    for k, (U, d) in enumerate(got):
        has(d, ["hadi_pass_a<1,1,"] + marks[k % 4], ["Bermudan", "barrier", "cliquet"] if k % 4 == 0 else [])
        checked("graph call %d" % k, U, refs[k % 4])
    for k in range(4):
        assert np.array_equal(got[k][0], got[k + 4][0])
