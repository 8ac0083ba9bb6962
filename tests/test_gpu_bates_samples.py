"""The Bates surface calls on the device (hadi_bates_sample_ladder, hadi_compute_base_prices_bates_samples,
hadi_compute_jacobian_bates_samples) on both routes, each pinned through "jump_small": 0 the streaming kernels followed by
hadi_jump_kernel / hadi_jump_sel_kernel and hadi_sample_kernel, 1 hadi_small_jump_kernel (the whole time loop in one launch, the
jump sub-step on the fp64 matrix core out of LDS).  The reference is tests/bates_samples_ref.py: jumps_ref.solve_batch at
N = snap_steps[q], then samples_ref.sample_batch.
Bounds, the project's: samples within 1e-10 sum|w| |scale| max|U_ref| on well-conditioned grids (asserted); base samples 1e-10
relative; J within 2e-4 sum|w| |scale| per column with eps = 1e-6 on rows of at most 100 nodes."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import bates_samples_ref as BS
import common as Cm
import samples_ref as SR

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
EPS = 1e-6
INVALID, UNSUPPORTED, NOT_ON_GRID = 1, 2, 4
N_STEPS, SNAPS = 6, [2, 5, 6]
STREAM, LOOP = 0, 1
LOOP_WORDS = "; Bates: jump sub-step on the fp64 matrix core inside the time loop"
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
SEL_WORDS = "; Bates: hadi_jump_sel_kernel (fp64 matrix core, three matrix sets picked by group) behind the last column pass of every step"
# per-instance jump laws, cycled through the batch; the third has intensity 0
LAM, MU, SIG = (0.5, 2.0, 0.0, 1.0, 0.3), (-0.10, -0.05, 0.05, -0.20, 0.10), (0.15, 0.10, 0.20, 0.25, 0.30)


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


@contextlib.contextmanager
def routed(sv, route):
    """The handle is shared by the session: the key goes back to its default."""
    sv.set_tuning("jump_small", route)
    try:
        yield
    finally:
        sv.set_tuning("jump_small", -1)


def names_the_route(d, route, n_snap, n_samp, sel=False):
    samp = "sampled ladder: %d snapshots x %d samples" % (n_snap, n_samp)
    if route == LOOP:
        return d.startswith("hadi_small_jump_kernel<") and d.endswith(samp + " evaluated inside the time loop" + LOOP_WORDS)
    return "row pass" in d and (samp + ", hadi_sample_kernel after each snapshot step") in d and d.endswith(SEL_WORDS if sel else JUMP_WORDS)


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False, same=False):
    """(strikes, grids, payoff, spots) on well-conditioned grids, built once per shape and left unchanged."""
    strikes = Cm.well_conditioned_strikes(m1, 1) * n if same else Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    spots = np.ascontiguousarray(np.stack([SR.kernel_test_spots(grids.Vec_s[k], Cm.S_0) for k in range(n)]))
    U0.setflags(write=False)
    spots.setflags(write=False)
    return strikes, grids, U0, spots


class Case:
    def __init__(self, m1, m2, n=3, N=N_STEPS, snaps=SNAPS, law=None, put=False, div=False, dts=None, same=False, scheme=0, theta=Cm.THETA):
        self.m1, self.m2, self.n, self.N, self.snaps, self.put, self.div, self.dts = m1, m2, n, N, list(snaps), put, div, dts
        self.scheme, self.theta = scheme, theta
        self.strikes, self.grids, self.U0, self.spots = batch(m1, m2, n, put, same)
        self.V_0 = Cm.v0_for(m2)
        self.law = laws(n) if law is None else law
        self._ref = {}

    def kw(self):
        per = {}
        if self.put:
            per.update(option_type=H.PUT, strikes=self.strikes)
        if self.dts:
            per["delta_t_i"] = self.dts
        return dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme,
                    per_instance=per or None)

    def ladder_kw(self):
        k = self.kw()
        per = k.pop("per_instance") or {}
        out = dict(k, per_instance={x: v for x, v in per.items() if x == "delta_t_i"} or None)
        if self.put:
            out.update(option_type=H.PUT, strikes=self.strikes)
        return out

    def ladder(self, sv, law=None, spots=None, snaps=None, **over):
        """bates_sample_ladder on the caller's v-grid."""
        out = sv.bates_sample_ladder(self.m1, self.m2, self.N, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F, *MODEL, self.grids, self.U0.copy(),
                                     self.spots if spots is None else spots, self.V_0, self.snaps if snaps is None else snaps,
                                     *(self.law if law is None else law), **{**self.ladder_kw(), **over})
        return out, sv.describe_last_sweep()

    def plain_ladder(self, sv):
        out = sv.sample_ladder(self.m1, self.m2, self.N, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F, *MODEL, self.grids, self.U0.copy(),
                               self.spots, self.V_0, self.snaps, **self.ladder_kw())
        return out, sv.describe_last_sweep()

    def head(self, spots=None):
        size = (self.m1 + 1) * (self.m2 + 1)
        return (self.spots if spots is None else spots, self.V_0, Cm.R_D, Cm.R_F) + MODEL + (self.m1, self.m2, size, self.N, self.theta,
                                                                                            Cm.T / self.N, self.n, self.grids)

    def jac(self, sv, cols8, law=None, **over):
        out = sv.compute_jacobian_bates_samples(*self.head(), self.U0.copy(), self.snaps, *(self.law if law is None else law),
                                                jump_columns=cols8, eps=EPS, **{**self.kw(), **over})
        return out + (sv.describe_last_sweep(),)

    def ref(self, law=None):
        """The reference's (values, sum|w| |scale|, max|U|) on the caller's v-grid: computed once per law, left unchanged."""
        law = self.law if law is None else law
        key = tuple(np.asarray(x, dtype=np.float64).tobytes() for x in law)
        if key not in self._ref:
            g = self.grids
            self._ref[key] = BS.sample_ladder(self.m1, self.m2, self.snaps, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v,
                                              g.Delta_s, g.Delta_v, self.U0, self.V_0, self.spots, None, *law,
                                              dividends=Cm.DIVS if self.div else None, put_strikes=self.strikes if self.put else None,
                                              scheme=self.scheme, dt_i=self.dts)
        return self._ref[key]

    def ref_jac(self, n_par, law=None):
        g = self.grids
        return BS.jacobian(self.m1, self.m2, self.snaps, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F, *MODEL, self.V_0, g.Vec_s, g.Delta_s,
                           self.U0, self.spots, None, *(self.law if law is None else law), n_par=n_par, eps=EPS,
                           dividends=Cm.DIVS if self.div else None, put_strikes=self.strikes if self.put else None)


def samples_within_bound(name, out, ref):
    vals, amp, top = ref
    bound = 1e-10 * amp * top[:, :, None]
    worst = (np.abs(out - vals) / bound).max()
    print("%s: worst |diff| / bound %.2e" % (name, worst))
    assert np.isfinite(out).all() and worst <= 1.0, (name, worst)


def jacobian_within_bounds(name, J, base, Jo, bo, amp):
    rel = np.abs(base - bo) / np.maximum(1.0, np.abs(bo))
    dj = (np.abs(J - Jo) / amp[..., None]).reshape(-1, J.shape[-1]).max(axis=0)
    print("%s: base %.2e relative, J per column / (sum|w| |scale|) %s" % (name, rel.max(), " ".join("%.1e" % x for x in dj)))
    assert np.isfinite(J).all() and rel.max() <= 1e-10 and dj.max() <= 2e-4, (name, rel.max(), dj)


# ---- the ladder on both routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_every_sample_is_within_the_bound(solver, route):
    case = Case(50, 25)
    with routed(solver, route):
        out, d = case.ladder(solver)
        assert out.shape == (3, 3, 10) and names_the_route(d, route, 3, 10), d
        samples_within_bound("50x25 route %d" % route, out, case.ref())
        # the instance with lambda = 0 is its plain solve on the same kernels: the streaming passes, or the block kernel of 8 wavefronts
        key, off = ("small_grid", 0) if route == STREAM else ("small_seq", 0)
        solver.set_tuning(key, off)
        try:
            plain, d0 = case.plain_ladder(solver)
        finally:
            solver.set_tuning(key, 1 if route == STREAM else -1)
        assert ("row pass" in d0) if route == STREAM else d0.startswith("hadi_small_kernel<1,8,EU>"), d0
        assert np.array_equal(out[2], plain[2]) and np.abs(out[0] - plain[0]).max() > 1e-6


def test_the_node_sample_is_compute_base_prices_bates_bit_for_bit(solver):
    """spots = [S_0], scale 1, snaps = [N] on the streaming route: the call is compute_base_prices_bates with another read-out."""
    case = Case(50, 25)
    size = (case.m1 + 1) * (case.m2 + 1)
    ws = H.DOWorkspace(case.n, size)
    with routed(solver, STREAM):
        ws.U[...] = case.U0
        out = solver.compute_base_prices_bates_samples(*case.head(spots=[Cm.S_0]), ws, [case.N], *case.law)
        d = solver.describe_last_sweep()
        assert np.array_equal(ws.U, case.U0) and names_the_route(d, STREAM, 1, 1), d
        want = solver.compute_base_prices_bates(Cm.S_0, *case.head()[1:], ws, *case.law)
        d1 = solver.describe_last_sweep()
    assert d1.endswith(JUMP_WORDS) and d1.split(";")[0] == d.split(";")[0], (d, d1)
    assert out.shape == (3, 1, 1) and np.array_equal(out[:, 0, 0], want)


@pytest.mark.parametrize("route", [STREAM, LOOP, -1], ids=["streaming", "whole-loop", "automatic"])
def test_zero_intensity_is_sample_ladder_bit_for_bit(solver, route):
    case = Case(50, 25)
    with routed(solver, route):
        out, d = case.ladder(solver, law=(0.0, -0.1, 0.15))
        plain, d0 = case.plain_ladder(solver)
        assert d == d0 and "Bates" not in d and np.array_equal(out, plain)
        out, d = case.ladder(solver, law=(np.zeros(3), MU[:3], SIG[:3]))
        assert d == d0 and np.array_equal(out, plain)


LAYOUTS = [(100, 12, 4), (200, 12, 3), (300, 12, 3), (600, 8, 2)]


@pytest.mark.parametrize("m1,m2,N", LAYOUTS, ids=["%dx%dx%d" % s for s in LAYOUTS])
def test_the_other_streaming_layouts(solver, m1, m2, N):
    case = Case(m1, m2, n=2, N=N, snaps=[1, N], law=laws(2))
    with routed(solver, STREAM):
        out, d = case.ladder(solver)
    assert names_the_route(d, STREAM, 2, 10), d
    samples_within_bound("%dx%d" % (m1, m2), out, case.ref())


@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
@pytest.mark.parametrize("m1,m2,N", [(50, 25, 6), (100, 12, 4)], ids=["50x25", "100x12"])
def test_puts_and_dividends(solver, route, m1, m2, N):
    case = Case(m1, m2, N=N, snaps=[2, N], put=True, div=True, law=laws(3, first=1))
    with routed(solver, route):
        out, d = case.ladder(solver)
    assert names_the_route(d, route, 2, 10), d
    samples_within_bound("DIV puts %dx%d route %d" % (m1, m2, route), out, case.ref())


@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_delta_t_i(solver, route):
    case = Case(50, 25, dts=[Cm.T / 6, 0.5 / 6, 0.8 / 6], div=True, law=laws(3, first=3))
    with routed(solver, route):
        out, d = case.ladder(solver)
    assert names_the_route(d, route, 3, 10), d
    samples_within_bound("delta_t_i route %d" % route, out, case.ref())


@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_shared_grid(solver, route):
    law = (np.array([0.5, 0.0, 2.0]), MU[0], SIG[0])
    case = Case(50, 25, same=True, law=law)
    with routed(solver, route):
        outs, d = case.ladder(solver, shared_grid=True)
        outp, _ = case.ladder(solver)
        assert names_the_route(d, route, 3, 10) and np.array_equal(outs, outp)
        samples_within_bound("shared route %d" % route, outs, case.ref(law=(law[0], np.full(3, MU[0]), np.full(3, SIG[0]))))
        with pytest.raises(H.HadiError) as e:  # a broken promise
            Case(50, 25, law=(0.5, -0.1, 0.15)).ladder(solver, shared_grid=True)
        assert e.value.status == INVALID
        again, _ = case.ladder(solver, shared_grid=True)
        assert np.array_equal(again, outs)


# ---- the Jacobian -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_jacobian_with_five_and_eight_columns(solver, route):
    case = Case(50, 25, n=2, law=(np.array([0.5, 0.0]), np.array([-0.10, 0.05]), np.array([0.15, 0.20])))
    with routed(solver, route):
        J8, b8, d8 = case.jac(solver, True)
        J5, b5, d5 = case.jac(solver, False)
    assert J8.shape == (2, 3, 10, 8) and b8.shape == (2, 3, 10) and J5.shape == (2, 3, 10, 5) and b5.shape == (2, 3, 10)
    assert names_the_route(d8, route, 3, 10, sel=True) and names_the_route(d5, route, 3, 10), (d8, d5)
    Jo, bo, amp = case.ref_jac(8)
    jacobian_within_bounds("8 columns route %d" % route, J8, b8, Jo, bo, amp)
    jacobian_within_bounds("5 columns route %d" % route, J5, b5, Jo[..., :5], bo, amp)
    # the same route: the first five columns and the base are the five-column call's bits
    assert d8.split(";")[0] == d5.split(";")[0], (d8, d5)
    assert np.array_equal(b8, b5) and np.array_equal(J8[..., :5], J5)
    # lambda_k = 0: the groups 7 and 8 are skipped as group 0 is -- exact zeros; the lambda column is not zero
    assert not J8[1, :, :, 6:].any() and (np.abs(J8[1, -1, :, 5]) > 0).any() and (np.abs(J8[0, -1, :, 5:]).max(axis=0) > 1e-4).all()


# ---- graph replay and handle reuse -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_call_a_then_a_larger_call_b_then_a_again(solver, route):
    A = Case(50, 25, n=2, N=4, snaps=[2, 4], law=laws(2))
    B = Case(100, 12, n=3, N=4, snaps=[1, 3, 4], law=laws(3, first=1), put=True)
    with routed(solver, route):
        a1, dA = A.ladder(solver)
        b1, dB = B.ladder(solver)
        a2, dA2 = A.ladder(solver)
        c0 = Cm.graph_counts(solver)
        a3, _ = A.ladder(solver)
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert dA == dA2 and names_the_route(dA, route, 2, 10) and names_the_route(dB, route, 3, 10)
    assert np.array_equal(a1, a2) and np.array_equal(a1, a3)
    if route == STREAM:
        assert delta["replays"] == 1 and delta["captures"] == 0, delta
    samples_within_bound("A", a1, A.ref())
    samples_within_bound("B", b1, B.ref())


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(solver):
    case = Case(50, 25)
    good = (0.5, -0.1, 0.15)
    ref, _ = case.ladder(solver, law=good)
    # the ladder's: N_i, call data with r_f != 0, a bad snapshot list, a spot off the grid
    assert status(case.ladder, solver, law=good, per_instance={"N_i": [6, 5, 6]}) == INVALID
    lad = lambda r_f: solver.bates_sample_ladder(case.m1, case.m2, case.N, Cm.T / case.N, Cm.THETA, Cm.R_D, r_f, *MODEL, case.grids,
                                                 case.U0.copy(), case.spots, case.V_0, case.snaps, *good)
    assert status(lad, 0.01) == UNSUPPORTED
    assert status(case.ladder, solver, law=good, snaps=[2, 2]) == INVALID and status(case.ladder, solver, law=good, snaps=[7]) == INVALID
    assert status(case.ladder, solver, law=good, spots=[1e9]) == NOT_ON_GRID
    # the jumps': the law, lambda dt > 1, American variants, grids that take the sequential passes
    for bad in ((-0.5, -0.1, 0.15), (0.5, -0.1, 0.0), (np.nan, -0.1, 0.15), (0.5, np.inf, 0.15), (6.5, -0.1, 0.15)):
        assert status(case.ladder, solver, law=bad) == INVALID, bad
    for variant in (H.AM, H.AM_DIV):
        assert status(case.ladder, solver, law=good, variant=variant, dividends=H.Dividends(*Cm.DIVS), U_0=case.U0) == UNSUPPORTED
    for m1, m2 in ((1100, 30), (40, 600)):
        seq = Case(m1, m2, n=1, N=2, snaps=[2], law=good)
        assert status(seq.ladder, solver) == UNSUPPORTED
    # the Jacobian: (lambda + eps) dt > 1 with eight columns only
    case.jac(solver, False, law=(6.0, -0.1, 0.15))
    assert status(case.jac, solver, True, law=(6.0, -0.1, 0.15)) == INVALID
    # the raw ABI: NULL structs, NULL outputs, the fp32 state, n_par
    lib, h = solver._lib, solver._h
    size = (case.m1 + 1) * (case.m2 + 1)
    jm, keep = solver._jumps(3, *good, False)
    st, keep2, n_samp = solver._samples(3, case.spots, None)
    steps = np.array(case.snaps, dtype=np.int32)
    sp = steps.ctypes.data_as(C.POINTER(C.c_int))
    p = solver._problem(H.EU, case.m1, case.m2, case.N, Cm.T / case.N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, case.grids, U=case.U0.copy())
    out = np.zeros((3, 3, n_samp))
    op = C.c_void_p(out.ctypes.data)
    for call in (lib.hadi_bates_sample_ladder, lib.hadi_compute_base_prices_bates_samples):
        assert call(h, C.byref(p), case.V_0, C.byref(st), 3, sp, None, op) == INVALID
        assert call(h, C.byref(p), case.V_0, None, 3, sp, C.byref(jm), op) == INVALID
        assert call(h, C.byref(p), case.V_0, C.byref(st), 3, sp, C.byref(jm), None) == INVALID
        assert call(h, C.byref(p), case.V_0, C.byref(st), 3, None, C.byref(jm), op) == INVALID
    p.state_precision = nat.STATE_FP32
    assert lib.hadi_bates_sample_ladder(h, C.byref(p), case.V_0, C.byref(st), 3, sp, C.byref(jm), op) == UNSUPPORTED
    p.state_precision = nat.STATE_FP64
    pj = solver._jacobian_problem(H.EU, Cm.R_D, Cm.R_F, *MODEL, case.m1, case.m2, size, case.N, Cm.THETA, Cm.T / case.N, case.grids,
                                  case.U0.copy(), None, None, 0)
    J, b = np.zeros((3, 3, n_samp, 8)), np.zeros((3, 3, n_samp))
    jp, bp = C.c_void_p(J.ctypes.data), C.c_void_p(b.ctypes.data)
    jc = lib.hadi_compute_jacobian_bates_samples
    for n_par in (0, 4, 6, 7, 9):
        assert jc(h, C.byref(pj), case.V_0, EPS, C.byref(st), 3, sp, C.byref(jm), n_par, jp, bp) == INVALID, n_par
    assert jc(h, C.byref(pj), case.V_0, EPS, C.byref(st), 3, sp, None, 8, jp, bp) == INVALID
    assert jc(h, C.byref(pj), case.V_0, EPS, C.byref(st), 3, sp, C.byref(jm), 8, None, bp) == INVALID
    assert jc(h, C.byref(pj), case.V_0, EPS, C.byref(st), 3, sp, C.byref(jm), 8, jp, None) == INVALID
    assert lib.hadi_version() == 2
    # and the handle still works
    assert lib.hadi_bates_sample_ladder(h, C.byref(p), case.V_0, C.byref(st), 3, sp, C.byref(jm), op) == 0
    assert np.array_equal(out, ref)
    assert jc(h, C.byref(pj), case.V_0, EPS, C.byref(st), 3, sp, C.byref(jm), 8, jp, bp) == 0 and np.isfinite(J).all()
    del keep, keep2


# ---- the calibration driver ---------------------------------------------------------------------------------------------------------------
class Checked:
    """The two launchers of calibrate_bates_surface on the GPU handle; every call is also made on the reference AT THE SAME
    PARAMETERS and held to the launchers' bounds there.  The loop sees the GPU's values."""

    def __init__(self, sv):
        self.sv, self.ref, self.calls = sv, BS.RefSolver(), 0

    def compute_jacobian_bates_samples(self, *a, **kw):
        J, base = self.sv.compute_jacobian_bates_samples(*a, **kw)
        Jo, bo = self.ref.compute_jacobian_bates_samples(*a, **kw)
        jacobian_within_bounds("loop Jacobian %d" % self.calls, J, base, Jo, bo, self.ref.last_amp)
        self.calls += 1
        return J, base

    def compute_base_prices_bates_samples(self, *a, **kw):
        p = self.sv.compute_base_prices_bates_samples(*a, **kw)
        po = self.ref.compute_base_prices_bates_samples(*a, **kw)
        rel = np.abs(p - po) / np.maximum(1.0, np.abs(po))
        print("loop trial %d: prices %.2e relative" % (self.calls, rel.max()))
        assert rel.max() <= 1e-10
        self.calls += 1
        return p


@pytest.mark.parametrize("route", [STREAM, LOOP], ids=["streaming", "whole-loop"])
def test_calibrate_bates_surface_one_iteration(solver, route):
    """The 6-strike x 3-maturity case of tests/test_calibration_bates_surface_cpu.py on the device: the Jacobian and the trial are
    held to the launchers' bounds where the loop stands, and the first trial parameters and errors are set beside the reference
    loop's at the tolerance tests/test_gpu_jumps8.py uses for calibrate_bates_jumps' trial error, 1e-4 relative."""
    grids, U0, market, start = BS.loop_case(H, Cm)
    want = BS.loop_run(H, Cm, BS.RefSolver(), grids, U0, market, start, max_iter=1)["history"][0]
    sv = Checked(solver)
    with routed(solver, route):
        res = BS.loop_run(H, Cm, sv, grids, U0, market, start, max_iter=1)
        d = solver.describe_last_sweep()
    got = res["history"][0]
    rel = [abs(a - b) / abs(b) for a, b in zip(got["trial"], want["trial"])]
    print("first trial parameters, relative difference to the reference loop's: %s; error %.6e vs %.6e, trial error %.6e vs %.6e"
          % (" ".join("%.1e" % x for x in rel), got["error"], want["error"], got["trial_error"], want["trial_error"]))
    assert sv.calls == 2 and res["iterations"] == 1 and res["pde_solves"] == 9 and names_the_route(d, route, 3, 6), d
    assert got["error"] == pytest.approx(want["error"], rel=1e-6) and got["trial_error"] < got["error"]
    assert got["trial_error"] == pytest.approx(want["trial_error"], rel=1e-4)
    assert max(rel) <= 1e-4, rel
