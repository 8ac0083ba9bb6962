"""Bermudan sweeps on the device (hadi_bermudan_timestepping, hadi_compute_base_prices_bermudan, hadi_compute_jacobian_bermudan):
one case per kernel that applies the exercise -- the four whole-loop LDS kernels and hadi_small_sch_kernel inside their time
loop, hadi_exercise_kernel behind the streaming kernels at every layout -- each with its tuning keys pinned and its kernel family
asserted from describe_last_sweep().  The reference is tests/bermudan_ref.py (oracle operators and line solves, the projection in
numpy); tests/test_bermudan_ref.py shows that a wrong schedule, a shifted one or a dropped date moves it by >= 1e-4 of max|U|.
Bounds: field 1e-10 of max|U_ref| on well-conditioned grids (asserted), prices 1e-9, J 2e-4.  No ordering against the European
field is asserted: the discrete scheme is not monotone."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import bermudan_ref as BR
import common as Cm

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "pair_strips": -1, "small_seq": -1,
            "small_pairs": -1, "small_sch": -1, "small_waves": 0, "streams": 0, "graph": 1}
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
EX_LOOP, EX_STREAM = "Bermudan: exercise at the end of", "hadi_exercise_kernel"
INVALID, UNSUPPORTED = 1, 2


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
    def __init__(self, m1, m2, n, N, ex, div=False, put=False, scheme=0, theta=Cm.THETA, N_i=None, dt_i=None):
        self.m1, self.m2, self.n, self.N, self.ex, self.div, self.put, self.scheme, self.theta = m1, m2, n, N, ex, div, put, scheme, theta
        self.N_i, self.dt_i = N_i, dt_i
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put)
        self.dt = Cm.T / N

    def kw(self):
        k = dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme)
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.N_i is not None:
            k["per_instance"] = {"N_i": self.N_i, "delta_t_i": self.dt_i}
        return k

    def head(self):
        return (self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F) + MODEL + (self.grids,)

    def run(self, sv, ex=None, U=None, **over):
        U = self.U0.copy() if U is None else U
        sv.bermudan_timestepping(*self.head(), U, self.ex if ex is None else ex, **{**self.kw(), **over})
        return U, sv.describe_last_sweep()

    def ref(self, ex=None, rows=None):
        g = self.grids
        return BR.solve_batch(self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v, g.Delta_s,
                              g.Delta_v, self.U0, self.ex if ex is None else ex, dividends=Cm.DIVS if self.div else None,
                              put_strikes=self.strikes if self.put else None, scheme=self.scheme, N_i=self.N_i, dt_i=self.dt_i,
                              rows=rows)


def field_check(name, U, Uo, rows=None):
    r = range(U.shape[0]) if rows is None else rows
    e = np.array([np.abs(U[k] - Uo[k]).max() / np.abs(Uo[k]).max() for k in r])
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
    check(solver, "%s %dx%d" % (name, m1, m2), Case(m1, m2, 3, 8, [2, 5, 8], put=put), tuning, [kernel % B, EX_LOOP + " 3 steps"],
          [EX_STREAM])


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("m1,m2,B", [(50, 25, 1), (100, 20, 2)], ids=["50x25", "100x20"])
def test_scheme_kernel(solver, scheme, theta, sname, m1, m2, B):
    check(solver, "small_sch %s %dx%d" % (sname, m1, m2), Case(m1, m2, 3, 6, [1, 4, 6], scheme=scheme, theta=theta), {"small_sch": 1},
          ["hadi_small_sch_kernel<%d,%s>" % (B, sname), EX_LOOP], [EX_STREAM])


# ---- hadi_exercise_kernel at every layout -------------------------------------------------------------------------------------
LAYOUTS = [("forced_streaming", 50, 25, 6, st(), ["hadi_pass_a<1,1,"]),
           ("two_per_lane", 100, 50, 4, st(), [("hadi_pass_a<2,1,", "hadi_pass_a_strip<2,")]),
           ("four_per_lane", 256, 128, 3, st(), [("hadi_pass_a<4,1,", "hadi_pass_a_strip<4,", "hadi_pass_a_pairs<")]),
           ("strips_eight_per_lane", 300, 80, 3, st(strip=1), ["hadi_pass_a_strip<8,EU>"]),
           ("two_wavefronts_per_row", 600, 30, 2, st(), [("hadi_pass_a<8,2,", "hadi_pass_a_strip<8,EU,double,2>")]),
           ("paired_strips", 600, 30, 2, st(strip=1), ["hadi_pass_a_strip<8,EU,double,2>"]),
           ("sequential_row_pass", 1100, 30, 2, st(), ["hadi_pass_a_seq<EU>"]),
           ("sequential_column_pass", 40, 600, 2, st(), ["hadi_pass_b_seq<EU>"]),
           ("m2_above_m1", 40, 60, 8, st(), ["hadi_pass_a<1,1,"])]


@pytest.mark.parametrize("name,m1,m2,N,tuning,want", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_exercise_kernel_layouts(solver, name, m1, m2, N, tuning, want):
    ex = sorted({max(1, N // 2), N})
    check(solver, name, Case(m1, m2, 3, N, ex, put=True), tuning, want + [EX_STREAM + " after each of %d exercise steps" % len(ex)],
          [EX_LOOP])


# ---- routing: never the team launch, never the resident sweep, sub-batches on two streams -------------------------------------
def test_team_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 140, 4, 3, [1, 3], put=True)
    with tuned(solver, {"team_launch": 1}):
        U, d = case.run(solver)
        assert "hadi_team_kernel" not in d and "row pass" in d and EX_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:  # (eligibility itself: the plain call of the same batch takes the team)
            _, d0 = case.run(solver, ex=[])
            assert "hadi_team_kernel" in d0 and "Bermudan" not in d0, d0
    field_check("team-eligible", U, case.ref(rows=[0, 3]), [0, 3])


def test_resident_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 80, 256, 2, [1, 2])
    with tuned(solver, {"resident_sweep": 1, "strip": 1}):
        U, d = case.run(solver)
        assert "hadi_sweep_resident" not in d and "hadi_pass_a_strip<8,EU>" in d and EX_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:
            _, d0 = case.run(solver, ex=[])
            assert "hadi_sweep_resident" in d0 and "Bermudan" not in d0, d0
    rows = [0, 100, 255]
    field_check("resident-eligible", U, case.ref(rows=rows), rows)


def test_sub_batches_on_two_streams(solver):
    """512x256 x 320 = a round of 256 and a remainder of 64: each sub-batch launches the exercise on its own stream, with its own
    offset into U, the payoff and the table (per-instance rows: odd instances exercise at step 2, even ones never)."""
    n, N = 320, 3
    ex = [[2] if k % 2 else [] for k in range(n)]
    case = Case(512, 256, n, N, ex, put=True)
    U, d = case.run(solver)
    assert "sub-batches" in d and "two streams" in d and EX_STREAM in d, d
    rows = [0, 255, 257, 319]
    Uo = case.ref(rows=rows)
    field_check("two streams", U, Uo, rows)
    plain = case.ref(ex=[], rows=[255])
    assert np.abs(Uo[255] - plain[255]).max() / np.abs(Uo[255]).max() >= 1e-4  # (the schedule matters at this N)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning,want", [("ring", 50, 25, st(small_sch=0), "hadi_pass_a"),
                                                     ("strips", 300, 80, st(small_sch=0, strip=1), "strip")], ids=["ring", "strips"])
def test_schemes_on_the_streaming_path(solver, scheme, theta, sname, path, m1, m2, tuning, want):
    check(solver, "%s %s" % (path, sname), Case(m1, m2, 2, 4, [2, 4], scheme=scheme, theta=theta), tuning, [want, sname, EX_STREAM],
          ["hadi_small_sch_kernel"])


PER_INSTANCE = [("block", {"small_seq": 0}, "hadi_small_kernel<"), ("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<"),
                ("seq2", {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"), ("streaming", st(), EX_STREAM)]


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
def test_per_instance_schedules_with_rotated_step_grids(solver, name, tuning, want):
    """Five instances, each with its own (N_i, dt_i) and its own schedule (one with none, one exercising at its own N_i): the
    pairs kernel holds instances of different N and different schedules in one wavefront."""
    N_i = [8, 5, 7, 3, 6]
    dt_i = [Cm.T / 8, 0.5 / 5, 0.8 / 7, 0.25 / 3, 0.6 / 6]
    ex = [[2, 8], [1, 3, 5], [], [3], [4]]
    check(solver, "per-instance " + name, Case(50, 25, 5, 8, ex, put=True, N_i=N_i, dt_i=dt_i), tuning, [want, "Bermudan"])


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_dividend_and_exercise_on_one_step(solver, name, tuning, want, put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16; the schedule exercises at the END of 8 and 16."""
    assert BR.dividend_steps(20, Cm.T / 20, Cm.DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}
    check(solver, "dividend step " + name, Case(50, 25, 3, 20, [8, 13, 16], div=True, put=put), tuning, [want, "Bermudan"])


def test_device_memory_inputs(solver):
    import torch
    case = Case(50, 25, 3, 6, [2, 6], put=True)
    dev = torch.device("cuda", 0)
    for tuning in ({"small_seq": 0}, st()):
        with tuned(solver, tuning):
            host, _ = case.run(solver)
            U = torch.from_numpy(case.U0.copy()).to(dev)
            solver.bermudan_timestepping(*case.head()[:-1], case.grids.to(dev), U, case.ex, **case.kw())
            assert np.array_equal(U.cpu().numpy(), host)
    field_check("device memory", host, case.ref())


def test_explicit_payoff_differs_from_the_initial_field(solver):
    """U_0 given: the exercise value is U_0, not the initial U (here the initial U is half the payoff); U_0 = NULL: the initial U."""
    case = Case(50, 25, 3, 6, [2, 6], put=True)
    g = case.grids
    for tuning in ({"small_seq": 1, "small_pairs": 0}, st()):
        with tuned(solver, tuning):
            U, _ = case.run(solver, U=0.5 * case.U0, U_0=case.U0.copy())
        Uo = BR.solve_batch(case.m1, case.m2, case.N, case.dt, case.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v, g.Delta_s,
                            g.Delta_v, 0.5 * case.U0, case.ex, payoff=case.U0, put_strikes=case.strikes)
        field_check("explicit payoff", U, Uo)


# ---- the launchers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,tuning,want", [(50, 25, {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"),
                                               (50, 25, st(), EX_STREAM), (128, 64, st(), EX_STREAM)],
                         ids=["50x25-lds", "50x25-streaming", "128x64-streaming"])
def test_launchers(solver, m1, m2, tuning, want):
    n, N, eps = 3, 6, 1e-6
    strikes, grids, U0 = batch(m1, m2, n, True)
    ex = [[2, 6], [3], [1, 4, 6]]
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    refkw = dict(put_strikes=strikes, V_0_i=v0s)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, ex)
    with tuned(solver, tuning):
        prices = solver.compute_base_prices_bermudan(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                     grids, ws, ex, per_instance=per)
        assert want in solver.describe_last_sweep() and "Bermudan" in solver.describe_last_sweep()
        J, base = solver.compute_jacobian_bermudan(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                   grids, U0.copy(), ex, eps=eps, per_instance=per)
        assert want in solver.describe_last_sweep() and "Bermudan" in solver.describe_last_sweep()
    po, Fo = BR.base_prices(*args, **refkw)
    Jo, bo = BR.jacobian(*args, eps=eps, **refkw)
    print("launchers %dx%d: prices %.2e, J %.2e" % (m1, m2, np.abs(prices - po).max(), np.abs(J - Jo).max()))
    field_check("launcher field", ws.U, Fo)
    assert np.abs(prices - po).max() <= 1e-9 and np.abs(base - bo).max() <= 1e-9
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


class RefSolver:
    """The two Bermudan launchers on tests/bermudan_ref.py, for the LM loop."""

    def __init__(self, strikes):
        self.strikes = strikes

    def _a(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U, ex):
        return (m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, grids.Vec_s, grids.Delta_s, np.asarray(U), ex)

    def compute_jacobian_bermudan(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, U_0, ex,
                                  eps=1e-6, **kw):
        return BR.jacobian(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U_0, ex), eps=eps)

    def compute_base_prices_bermudan(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, ws,
                                     ex, **kw):
        return BR.base_prices(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, ws.U, ex))[0]


def test_calibrate_bermudan_two_iterations(solver):
    """The LM loop over the Bermudan launchers against the same loop driven by the reference: same iterates to the launchers'
    bounds (the parameter updates divide J^T r by J^T J: 1e-6 on parameters of order 1 is three orders above what 2e-4 on J
    entries of order 10 .. 100 and 1e-9 on prices give)."""
    m1, m2, n, N = 50, 25, 4, 8
    strikes, grids, U0 = batch(m1, m2, n, False)
    ex = [2, 4, 6, 8]
    start = (Cm.KAPPA * 1.1, Cm.ETA * 0.9, Cm.SIGMA * 1.1, Cm.RHO * 0.9, Cm.V_0)
    size = (m1 + 1) * (m2 + 1)
    market = BR.base_prices(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, ex)[0]
    assert size == U0.shape[1]
    out = {}
    for name, sv in (("gpu", solver), ("ref", RefSolver(strikes))):
        out[name] = H.calibrate_bermudan(sv, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, *start, m1, m2, N, Cm.THETA, grids, U0.copy(), market, ex,
                                         max_iter=2, tol=1e-12)
    assert "Bermudan" in solver.describe_last_sweep()
    a, b = out["gpu"], out["ref"]
    assert a["iterations"] == b["iterations"] == 2
    for key in ("kappa", "eta", "sigma", "rho", "v0"):
        assert abs(a[key] - b[key]) <= 1e-6, (key, a[key], b[key])
    assert np.abs(a["model_prices"] - b["model_prices"]).max() <= 1e-6


# ---- identity and refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{}, {"small_seq": 1, "small_pairs": 1}, st(), st(strip=1)], ids=["default", "seq2", "ring", "strips"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 30)], ids=["50x25", "100x30"])
def test_empty_schedule_is_DO_timestepping_bit_for_bit(solver, tuning, m1, m2):
    case = Case(m1, m2, 3, 5, [])
    with tuned(solver, tuning):
        U, d = case.run(solver)
        V = case.U0.copy()
        solver.DO_timestepping(*case.head(), V)
        assert d == solver.describe_last_sweep() and "Bermudan" not in d, d
        assert np.array_equal(U, V)
        W, d2 = case.run(solver, ex=[[], [], []])  # a ragged schedule in which nobody has a date
        assert np.array_equal(W, V) and d2 == d


def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(solver):
    case = Case(50, 25, 3, 6, [2, 6])
    bt, head, U0 = solver.bermudan_timestepping, case.head(), case.U0
    for bad in ([0, 3], [3, 3], [4, 2], [7], [-1], [2, 0, 4], [[2], [7], [1]], [[2, 4], [4, 2], [1]]):
        assert status(bt, *head, U0.copy(), bad) == INVALID, bad
    # one schedule for a batch of mixed N_i: every entry within every instance's N_k
    per = {"N_i": [6, 4, 5], "delta_t_i": [Cm.T / 6] * 3}
    assert status(bt, *head, U0.copy(), [2, 5], per_instance=per) == INVALID
    bt(*head, U0.copy(), [2, 4], per_instance=per)
    assert status(bt, *head, U0.copy(), [[2, 6], [5], [1]], per_instance=per) == INVALID  # instance 1 has 4 steps
    for variant in (H.AM, H.AM_DIV):
        assert status(bt, *head, U0.copy(), [2], variant=variant, U_0=U0.copy(), dividends=H.Dividends(*Cm.DIVS)) == UNSUPPORTED
    # what check_problem refuses keeps its status: a scheme with dividends, MCS at theta = 0
    assert status(bt, *head, U0.copy(), [2], variant=H.DIV, dividends=H.Dividends(*Cm.DIVS), scheme=H.SCHEME_MCS) == UNSUPPORTED
    # the raw ABI: ex_rows, n_ex < 0, NULL steps, the fp32 state, NULL outputs
    lib, h = solver._lib, solver._h
    steps = np.array([2, 6, 2, 6], dtype=np.int32)
    sp = steps.ctypes.data_as(C.POINTER(C.c_int))
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())
    assert lib.hadi_bermudan_timestepping(h, C.byref(p), 2, sp, 2) == INVALID
    assert lib.hadi_bermudan_timestepping(h, C.byref(p), 2, sp, 0) == INVALID
    assert lib.hadi_bermudan_timestepping(h, C.byref(p), -1, sp, 1) == INVALID
    assert lib.hadi_bermudan_timestepping(h, C.byref(p), 2, None, 1) == INVALID
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_bermudan_timestepping(h, C.byref(p32), 2, sp, 1) == UNSUPPORTED
    pv = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_base_prices_bermudan(h, C.byref(pv), Cm.S_0, Cm.V_0, 2, sp, 1, None) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    out = np.zeros(3)
    assert lib.hadi_compute_jacobian_bermudan(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, 2, sp, 1, None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_jacobian_bermudan(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, 2, sp, 3, None, None) == INVALID
    # and the handle still works
    assert lib.hadi_bermudan_timestepping(h, C.byref(p), 2, sp, 1) == 0
    field_check("after the refusals", case.run(solver)[0], case.ref())


def test_exercise_steps_from_dates():
    assert H.exercise_steps(1.0, 0.05, [0.0, 0.25, 0.5, 0.75]) == [5, 10, 15, 20]
    assert H.exercise_steps(1.0, 1.0 / 12, [k / 12 for k in range(12)]) == list(range(1, 13))
    for bad in ([0.26], [1.0], [-0.05], [0.25, 0.25]):
        with pytest.raises(ValueError):
            H.exercise_steps(1.0, 0.05, bad)


# ---- graph cache --------------------------------------------------------------------------------------------------------------
def test_graph_cache_two_schedules_alternating(solver):
    """A, B, A on one handle: two captures and one replay, each result its own schedule's."""
    case = Case(50, 25, 3, 6, None, put=True)
    A, B = [2, 6], [3, 6]  # (same length, same number of exercise steps: only the steps differ)
    UA, UB = case.ref(ex=A), case.ref(ex=B)
    assert np.abs(UA - UB).max() / np.abs(UA).max() >= 1e-4
    with tuned(solver, st(graph=1)):
        case.run(solver, ex=[1, 5])  # (the buffers this shape needs are grown: growing one would empty the cache)
        c0 = Cm.graph_counts(solver)
        got = [case.run(solver, ex=e) for e in (A, B, A)]
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert all(EX_STREAM in d for _, d in got)
    assert (delta["captures"], delta["replays"]) == (2, 1), delta
    field_check("A", got[0][0], UA)
    field_check("B", got[1][0], UB)
    field_check("A again", got[2][0], UA)
    assert np.array_equal(got[0][0], got[2][0])
