"""Knock-out barrier sweeps on the device (hadi_barrier_timestepping, hadi_compute_base_prices_barrier,
hadi_compute_jacobian_barrier): one case per kernel that applies the knock-out -- the four whole-loop LDS kernels and
hadi_small_sch_kernel inside their time loop, hadi_knockout_kernel behind the streaming kernels at every layout -- each with its
tuning keys pinned and its kernel family asserted from describe_last_sweep().  The reference is tests/barrier_ref.py (oracle
operators and line solves, the knock-out in numpy); tests/test_barrier_ref.py shows that another instance's barrier, a shifted
schedule, a dropped date, a one-sided barrier, a forgotten rebate or `<` for `<=` moves it by >= 1e-4 of max|U|.
Bounds (those of tests/test_gpu_bermudan.py): field 1e-10 of the instance's max|U_ref| on well-conditioned grids (asserted),
prices 1e-9, J 2e-4.  No ordering against the vanilla field is asserted: the discrete scheme is not monotone."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import barrier_ref as KR
import bermudan_ref as BR
import common as Cm
from test_gpu_bermudan import LAYOUTS

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "pair_strips": -1, "small_seq": -1,
            "small_pairs": -1, "small_sch": -1, "small_waves": 0, "streams": 0, "graph": 1}
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
KO_LOOP, KO_STREAM = "barrier: knock-out at the end of", "barrier: hadi_knockout_kernel after each of"
INVALID, UNSUPPORTED = 1, 2
# per-instance double barriers (fractions of the instance's strike) and rebates, cycled through the batch
LOF, UPF, REB = (0.7, 0.8, 0.6, 0.75, 0.65), (1.3, 1.2, 1.4, 1.25, 1.5), (0.0, 1.5, 0.25, 3.0, 0.5)


class tuned:
    """Tuning keys for the block; every one goes back to its default on the way out (the handle is the session's)."""

    def __init__(self, sv, tuning):
        self.sv, self.tuning = sv, tuning

    def __enter__(self):
        for k, v in self.tuning.items():
            self.sv.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.tuning:
            self.sv.set_tuning(k, DEFAULTS[k])


def st(**tuning):
    return {**STREAMING, **tuning}


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False):
    """(strikes, grids, payoff) on well-conditioned grids, built once per shape and left unchanged."""
    strikes = Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0


class Case:
    def __init__(self, m1, m2, n, N, mon, div=False, put=False, scheme=0, theta=Cm.THETA, N_i=None, dt_i=None, bar=None):
        self.m1, self.m2, self.n, self.N, self.mon, self.div, self.put, self.scheme, self.theta = m1, m2, n, N, mon, div, put, scheme, theta
        self.N_i, self.dt_i = N_i, dt_i
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put)
        self.dt = Cm.T / N
        k = np.asarray(self.strikes)
        cyc = lambda t: np.array([t[i % 5] for i in range(n)])
        self.bar = (cyc(LOF) * k, cyc(UPF) * k, cyc(REB)) if bar is None else bar

    def kw(self):
        k = dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme)
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.N_i is not None:
            k["per_instance"] = {"N_i": self.N_i, "delta_t_i": self.dt_i}
        return k

    def head(self):
        return (self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F) + MODEL + (self.grids,)

    def run(self, sv, mon=None, U=None, bar=None, **over):
        U = self.U0.copy() if U is None else U
        lo, up, reb = self.bar if bar is None else bar
        sv.barrier_timestepping(*self.head(), U, self.mon if mon is None else mon, lower=lo, upper=up, rebate=reb, **{**self.kw(), **over})
        return U, sv.describe_last_sweep()

    def ref(self, mon=None, rows=None, bar=None):
        g = self.grids
        return KR.solve_batch(self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v, g.Delta_s,
                              g.Delta_v, self.U0, self.mon if mon is None else mon, *(self.bar if bar is None else bar),
                              dividends=Cm.DIVS if self.div else None, put_strikes=self.strikes if self.put else None,
                              scheme=self.scheme, N_i=self.N_i, dt_i=self.dt_i, rows=rows)


def field_check(name, U, Uo, rows=None):
    r = range(U.shape[0]) if rows is None else rows
    # (a reference field that is zero throughout -- nothing alive and no rebate -- must be met exactly: 0 / 0 counts as 0)
    e = np.array([np.abs(U[k] - Uo[k]).max() / np.abs(Uo[k]).max() if np.abs(Uo[k]).max() > 0 or np.abs(U[k]).max() > 0 else 0.0
                  for k in r])
    print("%s: field error %.3e of max|U_ref|" % (name, e.max()))
    assert np.isfinite(e).all() and e.max() <= 1e-10, (name, e)


def check(sv, name, case, tuning, want, absent=(), rows=None):
    with tuned(sv, tuning):
        U, d = case.run(sv)
    for w in want:
        assert any(x in d for x in ((w,) if isinstance(w, str) else w)), (w, d)
    for a in absent:
        assert a not in d, (a, d)
    field_check(name, U, case.ref(rows=rows), rows)
    return U, d


# ---- the whole-loop LDS kernels, by tuning key, on 50x25 and 100x20 -----------------------------------------------------------
SMALL = [("block8", {"small_seq": 0, "small_waves": 8}, "hadi_small_kernel<%d,8,EU>"),
         ("block4", {"small_seq": 0, "small_waves": 4}, "hadi_small_kernel<%d,4,EU>"),
         ("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<%d>"),
         ("seq2", {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<%d>")]


@pytest.mark.parametrize("m1,m2,B", [(50, 25, 1), (100, 20, 2)], ids=["50x25", "100x20"])
@pytest.mark.parametrize("name,tuning,kernel", SMALL, ids=[s[0] for s in SMALL])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_whole_loop_kernels(solver, m1, m2, B, name, tuning, kernel, put):
    # (three instances: the pairs kernel's last block holds one; the last date is the valuation date, n = N)
    check(solver, "%s %dx%d" % (name, m1, m2), Case(m1, m2, 3, 8, [2, 5, 8], put=put), tuning, [kernel % B, KO_LOOP + " 3 steps"],
          [KO_STREAM])


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("m1,m2,B", [(50, 25, 1), (100, 20, 2)], ids=["50x25", "100x20"])
def test_scheme_kernel(solver, scheme, theta, sname, m1, m2, B):
    check(solver, "small_sch %s %dx%d" % (sname, m1, m2), Case(m1, m2, 3, 6, [1, 4, 6], scheme=scheme, theta=theta), {"small_sch": 1},
          ["hadi_small_sch_kernel<%d,%s>" % (B, sname), KO_LOOP], [KO_STREAM])


# ---- hadi_knockout_kernel at every layout of tests/test_gpu_bermudan.py -------------------------------------------------------
@pytest.mark.parametrize("name,m1,m2,N,tuning,want", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_knockout_kernel_layouts(solver, name, m1, m2, N, tuning, want):
    mon = sorted({max(1, N // 2), N})
    check(solver, name, Case(m1, m2, 3, N, mon, put=True), tuning, want + [KO_STREAM + " %d monitoring steps" % len(mon)], [KO_LOOP])


# ---- edge cases of the comparison, on one LDS kernel and on streaming ---------------------------------------------------------
EDGE_PATHS = [("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<"), ("streaming", st(), KO_STREAM)]


@pytest.mark.parametrize("name,tuning,want", EDGE_PATHS, ids=[p[0] for p in EDGE_PATHS])
def test_edge_cases_of_the_comparison(solver, name, tuning, want):
    """Five instances: (0) both barriers exactly on nodes: touching knocks out; (1) up-only with lower = -inf; (2) down-only with
    upper = +inf; (3) barriers outside the grid: the European instance's bits; (4) nothing alive: the field is the rebate."""
    m1, m2, n, N = 50, 25, 5, 4
    strikes, grids, U0 = batch(m1, m2, n, True)
    vs = grids.Vec_s
    i_lo, i_up = int(np.searchsorted(vs[0], 0.7 * strikes[0])), int(np.searchsorted(vs[0], 1.3 * strikes[0]))
    mid = 0.5 * (vs[4][m1 // 2] + vs[4][m1 // 2 + 1])
    lo = np.array([vs[0][i_lo], -np.inf, 0.8 * strikes[2], -1.0, mid - 1e-9])
    up = np.array([vs[0][i_up], 1.2 * strikes[1], np.inf, vs[3][m1] + 1.0, mid + 1e-9])
    reb = np.array([0.5, 0.0, 2.0, 7.0, 1.25])
    case = Case(m1, m2, n, N, [2, 4], put=True, bar=(lo, up, reb))
    U, _ = check(solver, "edges " + name, case, tuning, [want, "barrier"])
    Ur = U.reshape(n, m2 + 1, m1 + 1)
    assert (Ur[0][:, i_lo] == 0.5).all() and (Ur[0][:, i_up] == 0.5).all() and (Ur[0][:, i_lo + 1] != 0.5).all()
    assert (Ur[4] == 1.25).all()
    with tuned(solver, tuning):
        V = U0.copy()
        solver.DO_timestepping(*case.head(), V, option_type=H.PUT, strikes=strikes)
        assert np.array_equal(U[3], V[3]) and not np.array_equal(U[1], V[1])
        # one-sided barriers through NULL arrays: an up-only batch and a down-only batch
        for bar in ((None, up, reb), (lo, None, reb), (lo, up, None)):
            W, d = case.run(solver, bar=bar)
            assert want in d
            field_check("NULL array " + name, W, case.ref(bar=bar))


@pytest.mark.parametrize("name,tuning,want", EDGE_PATHS, ids=[p[0] for p in EDGE_PATHS])
def test_monitoring_on_every_step(solver, name, tuning, want):
    check(solver, "every step " + name, Case(50, 25, 3, 6, list(range(1, 7)), put=True), tuning, [want, "6 "])


PER_INSTANCE = [("block", {"small_seq": 0}, "hadi_small_kernel<"), ("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<"),
                ("seq2", {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"), ("streaming", st(), KO_STREAM)]


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
def test_per_instance_barriers_rebates_and_schedules_with_rotated_step_grids(solver, name, tuning, want):
    """Five instances, each with its own (N_i, dt_i), barriers, rebate and schedule (one with none, one monitored at its own
    N_i): the pairs kernel holds instances of different N and different schedules in one wavefront."""
    N_i = [8, 5, 7, 3, 6]
    dt_i = [Cm.T / 8, 0.5 / 5, 0.8 / 7, 0.25 / 3, 0.6 / 6]
    mon = [[2, 8], [1, 3, 5], [], [3], [4]]
    check(solver, "per-instance " + name, Case(50, 25, 5, 8, mon, put=True, N_i=N_i, dt_i=dt_i), tuning, [want, "barrier"])


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_dividend_and_knock_out_on_one_step(solver, name, tuning, want, put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16; the knock-out acts at the END of 8 and 16."""
    assert BR.dividend_steps(20, Cm.T / 20, Cm.DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}
    check(solver, "dividend step " + name, Case(50, 25, 3, 20, [8, 16], div=True, put=put), tuning, [want, "barrier"])


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning,want", [("ring", 50, 25, st(small_sch=0), "hadi_pass_a"),
                                                     ("strips", 300, 80, st(small_sch=0, strip=1), "strip")], ids=["ring", "strips"])
def test_schemes_on_the_streaming_path(solver, scheme, theta, sname, path, m1, m2, tuning, want):
    check(solver, "%s %s" % (path, sname), Case(m1, m2, 2, 4, [2, 4], scheme=scheme, theta=theta), tuning, [want, sname, KO_STREAM],
          ["hadi_small_sch_kernel"])


# ---- routing: never the team launch, never the resident sweep, sub-batches on two streams -------------------------------------
def test_team_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 140, 4, 3, [1, 3], put=True)
    with tuned(solver, {"team_launch": 1}):
        U, d = case.run(solver)
        assert "hadi_team_kernel" not in d and "row pass" in d and KO_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:  # (eligibility itself: the plain call of the same batch takes the team)
            _, d0 = case.run(solver, mon=[])
            assert "hadi_team_kernel" in d0 and "barrier" not in d0, d0
    field_check("team-eligible", U, case.ref(rows=[0, 3]), [0, 3])


def test_resident_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 80, 256, 2, [1, 2])
    with tuned(solver, {"resident_sweep": 1, "strip": 1}):
        U, d = case.run(solver)
        assert "hadi_sweep_resident" not in d and "hadi_pass_a_strip<8,EU>" in d and KO_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:
            _, d0 = case.run(solver, mon=[])
            assert "hadi_sweep_resident" in d0 and "barrier" not in d0, d0
    rows = [0, 100, 255]
    field_check("resident-eligible", U, case.ref(rows=rows), rows)


def test_sub_batches_on_two_streams(solver):
    """512x256 x 320 = a round of 256 and a remainder of 64: each sub-batch launches the knock-out on its own stream, with its own
    offset into U and the four tables (per-instance rows: odd instances are monitored at step 2, even ones never)."""
    n, N = 320, 3
    mon = [[2] if k % 2 else [] for k in range(n)]
    case = Case(512, 256, n, N, mon, put=True)
    U, d = case.run(solver)
    assert "sub-batches" in d and "two streams" in d and KO_STREAM in d, d
    rows = [0, 255, 257, 319]
    Uo = case.ref(rows=rows)
    field_check("two streams", U, Uo, rows)
    plain = case.ref(mon=[], rows=[255])
    assert np.abs(Uo[255] - plain[255]).max() / np.abs(Uo[255]).max() >= 1e-4  # (the schedule matters at this N)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def test_device_memory_inputs(solver):
    import torch
    case = Case(50, 25, 3, 6, [2, 6], put=True)
    dev = torch.device("cuda", 0)
    lo, up, reb = case.bar
    for tuning in ({"small_seq": 0}, st()):
        with tuned(solver, tuning):
            host, _ = case.run(solver)
            U = torch.from_numpy(case.U0.copy()).to(dev)
            solver.barrier_timestepping(*case.head()[:-1], case.grids.to(dev), U, case.mon, lower=lo, upper=up, rebate=reb, **case.kw())
            assert np.array_equal(U.cpu().numpy(), host)
    field_check("device memory", host, case.ref())


# ---- the launchers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,tuning,want", [(50, 25, {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"),
                                               (50, 25, st(), KO_STREAM), (128, 64, st(), KO_STREAM)],
                         ids=["50x25-lds", "50x25-streaming", "128x64-streaming"])
def test_launchers(solver, m1, m2, tuning, want):
    n, N, eps = 3, 6, 1e-6
    strikes, grids, U0 = batch(m1, m2, n, True)
    mon = [[2, 6], [3], [1, 4, 6]]
    k = np.asarray(strikes)
    lo, up, reb = np.array(LOF[:n]) * k, np.array(UPF[:n]) * k, np.array(REB[:n])
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    refkw = dict(put_strikes=strikes, V_0_i=v0s, lower=lo, upper=up, rebate=reb)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, mon)
    with tuned(solver, tuning):
        prices = solver.compute_base_prices_barrier(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                    grids, ws, mon, lower=lo, upper=up, rebate=reb, per_instance=per)
        assert want in solver.describe_last_sweep() and "barrier" in solver.describe_last_sweep()
        J, base = solver.compute_jacobian_barrier(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                  grids, U0.copy(), mon, lower=lo, upper=up, rebate=reb, eps=eps, per_instance=per)
        assert want in solver.describe_last_sweep() and "barrier" in solver.describe_last_sweep()
    po, Fo = KR.base_prices(*args, **refkw)
    Jo, bo = KR.jacobian(*args, eps=eps, **refkw)
    print("launchers %dx%d: prices %.2e, J %.2e" % (m1, m2, np.abs(prices - po).max(), np.abs(J - Jo).max()))
    field_check("launcher field", ws.U, Fo)
    assert np.abs(prices - po).max() <= 1e-9 and np.abs(base - bo).max() <= 1e-9
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


# ---- identity and refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{}, {"small_seq": 1, "small_pairs": 1}, st(), st(strip=1)], ids=["default", "seq2", "ring", "strips"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 30)], ids=["50x25", "100x30"])
def test_empty_schedule_is_DO_timestepping_bit_for_bit(solver, tuning, m1, m2):
    case = Case(m1, m2, 3, 5, [])
    with tuned(solver, tuning):
        U, d = case.run(solver)
        V = case.U0.copy()
        solver.DO_timestepping(*case.head(), V)
        assert d == solver.describe_last_sweep() and "barrier" not in d, d
        assert np.array_equal(U, V)
        W, d2 = case.run(solver, mon=[[], [], []])  # a ragged schedule in which nobody has a date
        assert np.array_equal(W, V) and d2 == d
        X, d3 = case.run(solver, bar=(None, None, None))  # no barrier at all is fine without monitoring steps
        assert np.array_equal(X, V) and d3 == d


def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(solver):
    case = Case(50, 25, 3, 6, [2, 6])
    bt, head, U0 = solver.barrier_timestepping, case.head(), case.U0
    lo, up, reb = case.bar
    ok = dict(lower=lo, upper=up, rebate=reb)
    for bad in ([0, 3], [3, 3], [4, 2], [7], [-1], [2, 0, 4], [[2], [7], [1]], [[2, 4], [4, 2], [1]]):
        assert status(bt, *head, U0.copy(), bad, **ok) == INVALID, bad
    # one schedule for a batch of mixed N_i: every entry within every instance's N_k
    per = {"N_i": [6, 4, 5], "delta_t_i": [Cm.T / 6] * 3}
    assert status(bt, *head, U0.copy(), [2, 5], per_instance=per, **ok) == INVALID
    bt(*head, U0.copy(), [2, 4], per_instance=per, **ok)
    assert status(bt, *head, U0.copy(), [[2, 6], [5], [1]], per_instance=per, **ok) == INVALID  # instance 1 has 4 steps
    # the barriers and the rebate
    nan3, inf3 = np.array([np.nan, 1.0, 1.0]), np.array([0.0, np.inf, 0.0])
    assert status(bt, *head, U0.copy(), [2], lower=nan3, upper=up) == INVALID
    assert status(bt, *head, U0.copy(), [2], lower=lo, upper=nan3 * up) == INVALID
    assert status(bt, *head, U0.copy(), [2], lower=lo, upper=up, rebate=nan3) == INVALID
    assert status(bt, *head, U0.copy(), [2], lower=lo, upper=up, rebate=inf3) == INVALID
    assert status(bt, *head, U0.copy(), [2], lower=up, upper=lo) == INVALID          # lower > upper
    assert status(bt, *head, U0.copy(), [2], lower=lo, upper=lo) == INVALID          # lower == upper
    assert status(bt, *head, U0.copy(), [2], lower=np.array([lo[0], np.inf, lo[2]]), upper=None) == INVALID  # +inf >= +inf
    assert status(bt, *head, U0.copy(), [2]) == INVALID                              # both arrays NULL with n_mon > 0
    for variant in (H.AM, H.AM_DIV):
        assert status(bt, *head, U0.copy(), [2], variant=variant, dividends=H.Dividends(*Cm.DIVS), **ok) == UNSUPPORTED
    # what check_problem refuses keeps its status: a scheme with dividends
    assert status(bt, *head, U0.copy(), [2], variant=H.DIV, dividends=H.Dividends(*Cm.DIVS), scheme=H.SCHEME_MCS, **ok) == UNSUPPORTED
    # the raw ABI: a NULL struct, mon_rows, n_mon < 0, NULL steps, the fp32 state, NULL outputs
    lib, h = solver._lib, solver._h
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())

    def barrier(n_mon, steps, rows):
        b, keep = solver._barrier(3, [], lo, up, reb)
        arr = None if steps is None else np.asarray(steps, dtype=np.int32)
        b.n_mon, b.mon_rows = n_mon, rows
        b.mon_steps = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int))
        return b, (keep, arr)

    assert lib.hadi_barrier_timestepping(h, C.byref(p), None) == INVALID
    for n_mon, steps, rows in ((2, [2, 6, 2, 6], 2), (2, [2, 6], 0), (-1, [2, 6], 1), (2, None, 1)):
        b, keep = barrier(n_mon, steps, rows)
        assert lib.hadi_barrier_timestepping(h, C.byref(p), C.byref(b)) == INVALID, (n_mon, steps, rows)
    good, keep = barrier(2, [2, 6], 1)
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_barrier_timestepping(h, C.byref(p32), C.byref(good)) == UNSUPPORTED
    pv = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_base_prices_barrier(h, C.byref(pv), Cm.S_0, Cm.V_0, C.byref(good), None) == INVALID
    out = np.zeros(3)
    assert lib.hadi_compute_base_prices_barrier(h, C.byref(pv), Cm.S_0, Cm.V_0, None, C.c_void_p(out.ctypes.data)) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_jacobian_barrier(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, C.byref(good), None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_jacobian_barrier(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, None, None, None) == INVALID
    assert lib.hadi_version() == 2
    # and the handle still works
    assert lib.hadi_barrier_timestepping(h, C.byref(p), C.byref(good)) == 0
    field_check("after the refusals", case.run(solver)[0], case.ref())


def test_helpers_monitoring_steps_and_knock_out_payoff():
    assert H.monitoring_steps(1.0, 0.05, [0.0, 0.25, 0.5, 0.75]) == [5, 10, 15, 20]
    for bad in ([0.26], [1.0], [-0.05], [0.25, 0.25]):
        with pytest.raises(ValueError):
            H.monitoring_steps(1.0, 0.05, bad)
    strikes, grids, U0 = batch(50, 25, 3, True)
    vs = grids.Vec_s
    lo, up = np.array([vs[0][10], 60.0, 70.0]), np.array([vs[0][40], 130.0, 140.0])
    P = H.knock_out_payoff(grids, U0, lo, up, rebate=[0.5, 0.0, 2.0]).reshape(3, 26, 51)
    for k in range(3):
        dead = KR.knocked_nodes(vs[k], lo[k], up[k])
        assert (P[k][:, dead] == [0.5, 0.0, 2.0][k]).all() and np.array_equal(P[k][:, ~dead], U0[k].reshape(26, 51)[:, ~dead])
    assert P[0][0, 10] == 0.5 and P[0][0, 40] == 0.5 and P[0][0, 11] == U0[0][11]  # touching knocks out
    assert np.array_equal(H.knock_out_payoff(grids, U0, None, None), U0)
    assert not U0.flags.writeable  # (the payoff itself is left alone)


# ---- graph cache --------------------------------------------------------------------------------------------------------------
def test_graph_cache_two_schedules_alternating(solver):
    """A, B, A on one handle: two captures and one replay, each result its own schedule's; then the first schedule with other
    barriers and rebates: the tables are uploaded again whatever the cache holds, so the result is the new barriers'."""
    case = Case(50, 25, 3, 6, None, put=True)
    A, B = [2, 6], [3, 6]  # (same length, same number of monitoring steps: only the steps differ)
    UA, UB = case.ref(mon=A), case.ref(mon=B)
    assert np.abs(UA - UB).max() / np.abs(UA).max() >= 1e-4
    k = np.asarray(case.strikes)
    other = (0.8 * k, 1.2 * k, np.array([2.0, 0.0, 1.0]))
    UC = case.ref(mon=A, bar=other)
    assert np.abs(UA - UC).max() / np.abs(UA).max() >= 1e-4
    with tuned(solver, st(graph=1)):
        case.run(solver, mon=[1, 5])  # (the buffers this shape needs are grown: growing one would empty the cache)
        c0 = Cm.graph_counts(solver)
        got = [case.run(solver, mon=e) for e in (A, B, A)]
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
        C_, dC = case.run(solver, mon=A, bar=other)
    assert all(KO_STREAM in d for _, d in got) and KO_STREAM in dC
    assert (delta["captures"], delta["replays"]) == (2, 1), delta
    field_check("A", got[0][0], UA)
    field_check("B", got[1][0], UB)
    field_check("A again", got[2][0], UA)
    assert np.array_equal(got[0][0], got[2][0])
    field_check("A with other barriers", C_, UC)
