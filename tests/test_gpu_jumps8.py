"""The eight-column Bates Jacobian on the device (hadi_compute_jacobian_bates_jumps: nine groups of one sweep, three matrix sets,
hadi_jump_sel_kernel), the LM functions at width 8 and calibrate_bates_jumps.  The reference is tests/jumps8_ref.py: nine calls of
jumps_ref.base_prices.
Bounds, the launchers' (tests/test_gpu_jumps.py): prices 1e-10 relative, J 2e-4 on all eight columns."""
import ctypes as C
import functools

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import common as Cm
import jumps8_ref as J8

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS = 1.0 / 3.0
EPS = 1e-6
INVALID, UNSUPPORTED = 1, 2
SEL_WORDS = "; Bates: hadi_jump_sel_kernel (fp64 matrix core, three matrix sets picked by group) behind the last column pass of every step"
OLD_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
# per-instance jump laws, cycled through the batch; the fifth has intensity 0
LAM, MU, SIG = (0.5, 2.0, 0.3, 1.0, 0.0), (-0.10, -0.05, 0.10, -0.20, 0.05), (0.15, 0.10, 0.30, 0.25, 0.20)


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False, same=False):
    """(strikes, grids, payoff) on well-conditioned grids, built once per shape and left unchanged."""
    strikes = Cm.well_conditioned_strikes(m1, 1) * n if same else Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0


class Case:
    def __init__(self, m1, m2, n, N, law=None, put=False, div=False, scheme=0, theta=Cm.THETA, v0_i=False, same=False, eps=EPS):
        self.m1, self.m2, self.n, self.N, self.put, self.div, self.scheme, self.theta = m1, m2, n, N, put, div, scheme, theta
        self.eps = eps
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put, same)
        self.V_0 = Cm.v0_for(m2)
        self.law = laws(n) if law is None else law
        self.v0s = None
        if v0_i:
            c = [x[1] for x in Cm.mixed_vgrid_candidates(m2, vary_vd=False)]
            self.v0s = [c[k % len(c)] for k in range(n)]

    def kw(self):
        per = {}
        if self.put:
            per.update(option_type=H.PUT, strikes=self.strikes)
        if self.v0s is not None:
            per["V_0_i"] = self.v0s
        return dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme,
                    per_instance=per or None)

    def head(self):
        size = (self.m1 + 1) * (self.m2 + 1)
        return (Cm.S_0, self.V_0, Cm.R_D, Cm.R_F) + MODEL + (self.m1, self.m2, size, self.N, self.theta, Cm.T / self.N, self.n, self.grids)

    def jac8(self, sv, law=None, **over):
        out = sv.compute_jacobian_bates_jumps(*self.head(), self.U0.copy(), *(self.law if law is None else law), eps=self.eps,
                                              **{**self.kw(), **over})
        return out + (sv.describe_last_sweep(),)

    def jac5(self, sv, law=None, **over):
        out = sv.compute_jacobian_bates(*self.head(), self.U0.copy(), *(self.law if law is None else law), eps=self.eps, **{**self.kw(), **over})
        return out + (sv.describe_last_sweep(),)

    def ref(self, law=None, rows=None):
        g = self.grids
        kw = dict(dividends=Cm.DIVS if self.div else None, put_strikes=self.strikes if self.put else None, scheme=self.scheme)
        if rows is not None:
            kw["rows"] = rows
        return J8.jacobian8(self.m1, self.m2, self.N, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F, *MODEL, Cm.S_0, self.V_0, g.Vec_s, g.Delta_s,
                            self.U0, *(self.law if law is None else law), eps=self.eps, V_0_i=self.v0s, **kw)


def within_bounds(name, J, base, Jo, bo, rows=None):
    r = slice(None) if rows is None else rows
    rel = np.abs(base[r] - bo[r]) / np.maximum(1.0, np.abs(bo[r]))
    dj = np.abs(J[r] - Jo[r]).max(axis=0)
    print("%s: prices %.2e relative, J per column %s" % (name, rel.max(), " ".join("%.1e" % x for x in dj)))
    assert np.isfinite(J[r]).all() and rel.max() <= 1e-10 and dj.max() <= 2e-4, (name, rel.max(), dj)


# The step of the differences.  A column's error is the two prices' rounding errors over eps, so the bound 2e-4 asks for prices that
# agree with the reference's to 2e-4 eps -- 2e-10 at eps = 1e-6 -- although the field bound of this kernel family, 1e-10 of max|U_ref|
# with max|U_ref| ~ 8 K ~ 700, allows 7e-8.  The 50 and 100 node rows keep well inside 2e-10.  The two-wavefront rows of 600 nodes
# do not: their line solves amplify the 1.1e-16 of fp64 by the diagonal dominance 1 + theta dt v s^2 / h^2 ~ 1e4 .. 1e5.  Measured
# with eps = 1e-6 on this shape: prices 4.7e-12 relative, the columns off by 3e-6 (lambda: same matrix, same rounding) .. 1.6e-3,
# i.e. bumped prices 1.6e-9 apart -- the five columns of hadi_compute_jacobian_bates, whose bits the eight-column call repeats here
# (test_first_five_columns_...), among them.  So this shape differences with 1e-4 (1.6e-9 / 1e-4 = 1.6e-5, a tenth of the bound); the
# reference takes the same step, so the truncation error is the same on both sides.
EPS_600 = 1e-4
CASES = {
    "50x25x7-puts-V0i": dict(m1=50, m2=25, n=7, N=6, put=True, v0_i=True),
    "100x12x3": dict(m1=100, m2=12, n=3, N=4),
    "600x8x2": dict(m1=600, m2=8, n=2, N=2, eps=EPS_600,
                    law=(np.array([0.3, 1.0]), np.array([0.10, -0.20]), np.array([0.30, 0.25]))),  # (dt = 1 / 2: lambda + eps <= 2)
    "50x25x4-DIV-puts": dict(m1=50, m2=25, n=4, N=6, put=True, div=True),
    "50x25x3-MCS": dict(m1=50, m2=25, n=3, N=5, scheme=H.SCHEME_MCS, theta=TH_MCS),
}


@pytest.mark.parametrize("name", list(CASES))
def test_jacobian_and_base_against_the_reference(solver, name):
    case = Case(**CASES[name])
    J, base, d = case.jac8(solver)
    assert J.shape == (case.n, 8) and base.shape == (case.n,) and d.endswith(SEL_WORDS), d
    Jo, bo = case.ref()
    within_bounds(name, J, base, Jo, bo)
    lam = case.law[0]
    for k in range(case.n):
        if lam[k] == 0.0:  # groups 7 and 8 are skipped as group 0 is: the same bits, exact zeros
            assert J[k, 6] == 0.0 and J[k, 7] == 0.0 and abs(J[k, 5]) > 1e-3, (k, J[k])
        else:
            assert (np.abs(J[k, 5:]) > 1e-4).all(), (k, J[k])
    if name == "50x25x7-puts-V0i":
        assert (lam == 0.0).sum() == 1


SAME_ROUTE = ("50x25x7-puts-V0i", "100x12x3", "600x8x2")  # 6 n and 9 n instances take the same pass kernels: bit-equal


@pytest.mark.parametrize("name,kw", [(k, CASES[k]) for k in SAME_ROUTE] + [("300x12x40", dict(m1=300, m2=12, n=40, N=3)),
                                                                         ("50x25x40", dict(m1=50, m2=25, n=40, N=4))],
                         ids=list(SAME_ROUTE) + ["300x12x40", "50x25x40"])
def test_first_five_columns_and_base_are_compute_jacobian_bates(solver, name, kw):
    """Bit for bit where both batches run the same pass kernels (the words of describe_last_sweep in front of the Bates clause
    agree): asserted to be so for the three SAME_ROUTE cases; the launchers' bounds otherwise."""
    case = Case(**kw)
    J8_, b8, d8 = case.jac8(solver)
    J5, b5, d5 = case.jac5(solver)
    assert d8.endswith(SEL_WORDS) and d5.endswith(OLD_WORDS)
    same = d8[:-len(SEL_WORDS)] == d5[:-len(OLD_WORDS)]
    print("%s: %s" % (name, "same pass kernels" if same else "%s | %s" % (d5[:120], d8[:120])))
    if name in SAME_ROUTE:
        assert same, (d5, d8)
    if same:
        assert np.array_equal(b8, b5) and np.array_equal(J8_[:, :5], J5)
    else:
        assert (np.abs(b8 - b5) / np.maximum(1.0, np.abs(b5))).max() <= 1e-10 and np.abs(J8_[:, :5] - J5).max() <= 2e-4


def test_shared_matrices(solver):
    """300x12 x 40 on one grid with a shared (mu_J, sigma_J) and per-instance intensities (every fifth: 0) -- the shape at which
    several instances ride on one staged strip of a shared matrix: three matrices for the batch give the bits of 120."""
    n = 40
    law = (np.array([LAM[(k + 3) % 5] for k in range(n)]), MU[0], SIG[0])
    case = Case(300, 12, n, 3, law=law, same=True)
    Js, bs, d = case.jac8(solver, shared_grid=True)
    Jp, bp, _ = case.jac8(solver)
    assert d.endswith(SEL_WORDS) and np.array_equal(Js, Jp) and np.array_equal(bs, bp)
    rows = [0, 1, n - 1]
    Jo, bo = case.ref(law=(law[0], np.full(n, MU[0]), np.full(n, SIG[0])), rows=rows)
    within_bounds("shared", Js, bs, Jo, bo, rows)
    assert np.array_equal(Js[0], Js[5]) and not np.array_equal(Js[0], Js[1])  # (same law, same grid: the same row)
    with pytest.raises(H.HadiError) as e:  # the promise is checked here as well
        Case(50, 25, 3, 3, law=(0.5, -0.1, 0.15)).jac8(solver, shared_grid=True)
    assert e.value.status == INVALID


def test_strip_sharing_changes_no_bit(solver):
    """"jump_share" 0 (one instance per block) against the default on per-instance matrices, at a batch large enough for strips of
    seven instances (50x25 x 150: 1350 instances, four 16-slot blocks each) and at one of two sub-batches."""
    for kw in (dict(m1=50, m2=25, n=150, N=3), dict(m1=256, m2=128, n=64, N=2)):
        case = Case(law=(0.5, -0.10, 0.15), **kw)
        J1, b1, d1 = case.jac8(solver)
        solver.set_tuning("jump_share", 0)
        try:
            J0, b0, d0 = case.jac8(solver)
        finally:
            solver.set_tuning("jump_share", 1)
        assert d0 == d1 and np.array_equal(J0, J1) and np.array_equal(b0, b1)
        assert np.isfinite(J1).all() and (np.abs(J1[:, 5:]) > 1e-4).all()


def test_lm_partials_device_at_width_8_and_5(solver):
    import torch
    dev = torch.device("cuda:0")
    n = 500
    rng = np.random.default_rng(8)
    market, model = rng.standard_normal(n) + 10.0, rng.standard_normal(n) + 10.0
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for w in (8, 5, 1):
        J = np.ascontiguousarray(rng.standard_normal((n, w)) * rng.uniform(0.1, 10.0, w))
        got = H.lm_partials_device(solver, td(J), td(model), td(market))
        want = H.lm_partials(J, market - model)
        # each sum is n products: the host adds them one by one (n u), the device by a tree of fma (a few u) -- relative to the
        # sum of the magnitudes, 500 x 1.1e-16 < 1e-13
        scale = H.lm_partials(np.abs(J), np.abs(market - model))
        assert got.shape == (w * w + w + 1,) and (np.abs(got - want) <= 1e-13 * scale).all(), w
        if w == 5:  # bit-equal to the five-parameter entry point, by either name
            a, b = np.empty(31), np.empty(31)
            Jd, md, kd = td(J), td(model), td(market)
            ptrs = (C.c_void_p(Jd.data_ptr()), C.c_void_p(md.data_ptr()), C.c_void_p(kd.data_ptr()))
            torch.cuda.synchronize()
            assert solver._lib.hadi_lm_partials_device(solver._h, n, *ptrs, a.ctypes.data_as(nat._dp)) == 0
            assert solver._lib.hadi_lm_partials_device_n(solver._h, n, 5, *ptrs, b.ctypes.data_as(nat._dp)) == 0
            assert np.array_equal(a, b) and np.array_equal(a, got)
    out = np.zeros(73)
    Jd = td(np.zeros((4, 8)))
    for bad in (0, 9, -1):
        assert solver._lib.hadi_lm_partials_device_n(solver._h, 4, bad, C.c_void_p(Jd.data_ptr()), C.c_void_p(Jd.data_ptr()),
                                                     C.c_void_p(Jd.data_ptr()), out.ctypes.data_as(nat._dp)) == INVALID


class Checked:
    """The two launchers of calibrate_bates_jumps on the GPU handle; every call is also made on the reference AT THE SAME
    PARAMETERS and held to the launchers' bounds there.  The loop sees the GPU's values."""

    def __init__(self, sv):
        self.sv, self.ref, self.calls = sv, J8.RefSolver8(), 0

    def compute_jacobian_bates_jumps(self, *a, **kw):
        J, base = self.sv.compute_jacobian_bates_jumps(*a, **kw)
        Jo, bo = self.ref.compute_jacobian_bates_jumps(*a, **kw)
        within_bounds("loop Jacobian %d" % self.calls, J, base, Jo, bo)
        self.calls += 1
        return J, base

    def compute_base_prices_bates(self, *a, **kw):
        ws = a[16]
        U_in = np.array(ws.U, copy=True)
        p = self.sv.compute_base_prices_bates(*a, **kw)
        ws.U = U_in
        po = self.ref.compute_base_prices_bates(*a, **kw)
        rel = np.abs(p - po) / np.maximum(1.0, np.abs(po))
        print("loop trial %d: prices %.2e relative" % (self.calls, rel.max()))
        assert rel.max() <= 1e-10
        self.calls += 1
        return p


def test_calibrate_bates_jumps_two_iterations(solver):
    """The twelve-strike case of tests/test_calibration_bates_jumps_cpu.py on the device.  No trajectory of another loop is compared
    (cond(J^T J) is 1e7 .. 1e9: it would measure conditioning): each Jacobian and trial is checked where the loop stands."""
    grids, U0, market, start = J8.loop_case(H, Cm)
    sv = Checked(solver)
    res = J8.loop_run(H, Cm, sv, grids, U0, market, start)
    hist = res["history"]
    print("sum r^2: %s -> final %.3e" % (" -> ".join("%.3e" % h["error"] for h in hist), res["final_error"]))
    assert sv.calls == 4 and "hadi_jump_kernel" in solver.describe_last_sweep()  # (the last call is a trial)
    assert res["iterations"] == 2 and all(h["trial_error"] < h["error"] for h in hist)  # both accepted, as on the reference
    assert res["final_error"] <= 1e-3
    assert res["pde_solves"] == 12 * 10 * 2 - 12
    # device-resident inputs: J stays on the device and the 73 sums are reduced there
    import torch
    dev = torch.device("cuda:0")
    rd = H.calibrate_bates_jumps(solver, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, *start[:5], J8.LOOP_M1, J8.LOOP_M2, J8.LOOP_N, Cm.THETA, grids.to(dev),
                                 torch.from_numpy(U0).to(dev), market, *start[5:], max_iter=1, tol=1e-12)
    h0 = rd["history"][0]
    assert h0["error"] == pytest.approx(hist[0]["error"], rel=1e-12) and h0["trial_error"] < h0["error"]
    assert h0["trial_error"] == pytest.approx(hist[0]["trial_error"], rel=1e-4)


def test_graph_replay_and_a_second_law(solver):
    case = Case(100, 12, 3, 6, put=True)
    lawB = laws(3, first=2)
    solver.set_tuning("graph", 1)
    case.jac8(solver)  # (the buffers this shape needs are grown: growing one would empty the cache)
    c0 = Cm.graph_counts(solver)
    JA, bA, dA = case.jac8(solver)
    JA2, bA2, dA2 = case.jac8(solver)
    JB, bB, _ = case.jac8(solver, law=lawB)
    JA3, bA3, _ = case.jac8(solver)
    delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert delta["replays"] >= 3 and delta["captures"] <= 1 and dA == dA2, delta
    assert np.array_equal(JA, JA2) and np.array_equal(bA, bA2) and np.array_equal(JA, JA3) and not np.array_equal(JA, JB)
    solver.set_tuning("graph", 0)
    try:
        JE, bE, _ = case.jac8(solver)
    finally:
        solver.set_tuning("graph", 1)
    assert np.array_equal(JA, JE) and np.array_equal(bA, bE)
    within_bounds("law B over the replayed loop", JB, bB, *case.ref(law=lawB))


def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(solver):
    case = Case(50, 25, 3, 6)
    jb, head, U0 = solver.compute_jacobian_bates_jumps, case.head(), case.U0
    # lambda dt = 1 is a law the five-column call admits; (lambda + eps) dt > 1 is not one for the lambda group
    solver.compute_jacobian_bates(*head, U0.copy(), 6.0, -0.1, 0.15, eps=EPS)
    assert status(jb, *head, U0.copy(), 6.0, -0.1, 0.15, eps=EPS) == INVALID
    assert status(jb, *head, U0.copy(), np.array([0.5, 6.0, 0.5]), -0.1, 0.15, eps=EPS) == INVALID
    jb(*head, U0.copy(), 6.0 - 2 * EPS, -0.1, 0.15, eps=EPS)
    for bad in ((-0.5, -0.1, 0.15), (0.5, -0.1, 0.0), (np.nan, -0.1, 0.15), (0.5, np.inf, 0.15), (6.5, -0.1, 0.15)):
        assert status(jb, *head, U0.copy(), *bad, eps=EPS) == INVALID, bad
    for variant in (H.AM, H.AM_DIV):
        assert status(jb, *head, U0.copy(), 0.5, -0.1, 0.15, variant=variant, dividends=H.Dividends(*Cm.DIVS)) == UNSUPPORTED
    for m1, m2 in ((1100, 30), (40, 600)):  # grids that take the sequential passes
        seq = Case(m1, m2, 1, 2, law=(0.5, -0.1, 0.15))
        assert status(seq.jac8, solver) == UNSUPPORTED
    # the raw ABI: a NULL struct, the fp32 state, NULL outputs
    lib, h = solver._lib, solver._h
    good, keep = solver._jumps(3, 0.5, -0.1, 0.15, False)
    size = (case.m1 + 1) * (case.m2 + 1)
    pj = solver._jacobian_problem(H.EU, Cm.R_D, Cm.R_F, *MODEL, case.m1, case.m2, size, case.N, Cm.THETA, Cm.T / case.N, case.grids,
                                  U0.copy(), None, None, 0)
    J, b = np.zeros((3, 8)), np.zeros(3)
    jp, bp = C.c_void_p(J.ctypes.data), C.c_void_p(b.ctypes.data)
    call = lib.hadi_compute_jacobian_bates_jumps
    assert call(h, C.byref(pj), Cm.S_0, case.V_0, EPS, None, jp, bp) == INVALID
    assert call(h, C.byref(pj), Cm.S_0, case.V_0, EPS, C.byref(good), None, bp) == INVALID
    assert call(h, C.byref(pj), Cm.S_0, case.V_0, EPS, C.byref(good), jp, None) == INVALID
    pj.state_precision = nat.STATE_FP32
    assert call(h, C.byref(pj), Cm.S_0, case.V_0, EPS, C.byref(good), jp, bp) == UNSUPPORTED
    pj.state_precision = nat.STATE_FP64
    assert lib.hadi_version() == 2
    # and the handle still works
    assert call(h, C.byref(pj), Cm.S_0, case.V_0, EPS, C.byref(good), jp, bp) == 0
    J2, b2, _ = case.jac8(solver, law=(0.5, -0.1, 0.15))
    assert np.array_equal(J, J2) and np.array_equal(b, b2)
    within_bounds("after the refusals", J2, b2, *case.ref(law=(0.5, -0.1, 0.15)))
