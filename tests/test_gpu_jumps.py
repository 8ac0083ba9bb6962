"""Bates sweeps on the device (hadi_bates_timestepping, hadi_compute_base_prices_bates, hadi_compute_jacobian_bates,
hadi_debug_jump_matrix): hadi_jump_matrix_kernel against the numpy generator, hadi_jump_kernel behind the streaming kernels at
every streaming layout (1, 2, 4, 8 nodes per lane, two wavefronts per row) and on the 512x256 shape the measurement runs on, the
three entry points, a shared matrix, the graph cache, handle reuse, the refusals, and zero intensity as the plain call.  The
reference is tests/jumps_ref.py (oracle operators and line solves, the generator and the sub-step in numpy);
tests/test_jumps_ref.py holds it to the semi-analytic Bates price and shows that each class of mistake in the generator moves
the price by more than 1e-2.
Bounds: field 1e-10 of the instance's max|U_ref| on well-conditioned grids (asserted), prices 1e-10 relative, J 2e-4 (the bound of
tests/test_gpu_barrier.py); matrix entries 1e-13 max(1, |kbar| s_i / min(ds_{i-1}, ds_i))."""
import ctypes as C
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import common as Cm
import jumps_ref as JR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "small_seq": -1, "small_pairs": -1, "small_sch": -1,
            "graph": 1}
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
INVALID, UNSUPPORTED = 1, 2
# per-instance jump laws, cycled through the batch: the three sets of the accuracy table, a fourth, and one with intensity 0
LAM, MU, SIG = (0.5, 2.0, 0.3, 1.0, 0.0), (-0.10, -0.05, 0.10, -0.20, 0.05), (0.15, 0.10, 0.30, 0.25, 0.20)


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


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False, same=False):
    """(strikes, grids, payoff) on well-conditioned grids, built once per shape and left unchanged.  same: every instance on
    instance 0's grid."""
    strikes = Cm.well_conditioned_strikes(m1, 1) * n if same else Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


class Case:
    def __init__(self, m1, m2, n, N, law=None, div=False, put=False, scheme=0, theta=Cm.THETA, N_i=None, dt_i=None, same=False):
        self.m1, self.m2, self.n, self.N, self.div, self.put, self.scheme, self.theta = m1, m2, n, N, div, put, scheme, theta
        self.N_i, self.dt_i = N_i, dt_i
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put, same)
        self.dt = Cm.T / N
        self.law = laws(n) if law is None else law

    def kw(self):
        k = dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme)
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.N_i is not None:
            k["per_instance"] = {"N_i": self.N_i, "delta_t_i": self.dt_i}
        return k

    def head(self):
        return (self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F) + MODEL + (self.grids,)

    def run(self, sv, law=None, U=None, **over):
        U = self.U0.copy() if U is None else U
        sv.bates_timestepping(*self.head(), U, *(self.law if law is None else law), **{**self.kw(), **over})
        return U, sv.describe_last_sweep()

    def plain(self, sv):
        U = self.U0.copy()
        sv.DO_timestepping(*self.head(), U, **self.kw())
        return U, sv.describe_last_sweep()

    def ref(self, law=None, rows=None):
        g = self.grids
        return JR.solve_batch(self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v, g.Delta_s,
                              g.Delta_v, self.U0, *(self.law if law is None else law), dividends=Cm.DIVS if self.div else None,
                              put_strikes=self.strikes if self.put else None, scheme=self.scheme, N_i=self.N_i, dt_i=self.dt_i, rows=rows)


def field_check(name, U, Uo, rows=None):
    r = range(U.shape[0]) if rows is None else rows
    e = np.array([np.abs(U[k] - Uo[k]).max() / np.abs(Uo[k]).max() for k in r])
    print("%s: field error %.3e of max|U_ref|" % (name, e.max()))
    assert np.isfinite(e).all() and e.max() <= 1e-10, (name, e)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", [50, 100, 200, 300, 512, 600])
def test_matrix_kernel_against_the_numpy_generator(solver, m1):
    vs = batch(m1, 8, 1)[1].Vec_s[0]
    ds = np.diff(vs)
    hmin = np.minimum(np.r_[ds[0], ds], np.r_[ds, ds[-1]])
    for lam, mu, sig in list(zip(LAM, MU, SIG))[:3]:
        G, Gr = solver.debug_jump_matrix(vs, mu, sig), JR.generator(vs, mu, sig)
        bound = 1e-13 * np.maximum(1.0, abs(JR.kbar(mu, sig)) * vs / hmin)
        worst = (np.abs(G - Gr) / bound[:, None]).max()
        print("m1 = %d (%g, %g): worst entry at %.3f of its bound" % (m1, mu, sig, worst))
        assert np.isfinite(G).all() and worst <= 1.0 and not G[0].any()
        assert np.abs(G @ np.ones(m1 + 1)).max() <= 1e-12 * vs.max() and np.abs(G @ vs).max() <= 1e-12 * vs.max()


# ---- the five streaming layouts, through the C ABI ---------------------------------------------------------------------------------------
LAYOUTS = [("one_per_lane", 50, 25, 8, ["hadi_pass_a<1,1,"]),
           ("two_per_lane", 100, 12, 6, [("hadi_pass_a<2,1,", "hadi_pass_a_strip<2,")]),
           ("four_per_lane", 200, 12, 4, [("hadi_pass_a<4,1,", "hadi_pass_a_strip<4,", "hadi_pass_a_pairs<")]),
           ("eight_per_lane", 300, 12, 3, [("hadi_pass_a<8,1,", "hadi_pass_a_strip<8,")]),
           ("two_wavefronts_per_row", 600, 8, 2, [("hadi_pass_a<8,2,", "hadi_pass_a_strip<8,EU,double,2>")])]


@pytest.mark.parametrize("put,div", [(False, False), (True, True)], ids=["EU-call", "DIV-put"])
@pytest.mark.parametrize("name,m1,m2,N,want", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_jump_kernel_layouts(solver, name, m1, m2, N, want, put, div):
    """Five instances with their own jump laws, the last with intensity 0: it is its plain solve bit for bit."""
    case = Case(m1, m2, 5, N, put=put, div=div)
    U, d = case.run(solver)
    for w in want:
        assert any(x in d for x in ((w,) if isinstance(w, str) else w)), (w, d)
    assert d.endswith(JUMP_WORDS) and "hadi_small" not in d and "hadi_team" not in d and "hadi_sweep_resident" not in d, d
    Uo = case.ref()
    field_check(name, U, Uo)
    with tuned(solver, {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}):
        P, _ = case.plain(solver)
    assert np.array_equal(U[4], P[4])
    assert all(np.abs(U[k] - P[k]).max() > 1e-6 * np.abs(Uo[k]).max() for k in range(4))


@pytest.mark.parametrize("scheme,theta", [(H.SCHEME_CRAIG_SNEYD, 0.5), (H.SCHEME_MCS, TH_MCS), (H.SCHEME_HV, TH_HV)], ids=["CS", "MCS", "HV"])
@pytest.mark.parametrize("m1,m2,N", [(50, 25, 5), (300, 12, 3)], ids=["50x25", "300x12"])
def test_schemes(solver, scheme, theta, m1, m2, N):
    case = Case(m1, m2, 3, N, scheme=scheme, theta=theta)
    U, d = case.run(solver)
    assert d.endswith(JUMP_WORDS), d
    field_check("scheme %d" % scheme, U, case.ref())


N_MIX = [5, 8, 3, 7, 6]
DT_MIX = [0.5 / 5, Cm.T / 8, 0.25 / 3, 0.8 / 7, 0.6 / 6]


@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (200, 12)])
def test_mixed_step_grids_models_and_jump_laws(solver, m1, m2, div):
    """Every instance its own (N, dt), jump law and dividend dating; a one-instance call equals the same instance inside the batch of
    five bit for bit."""
    case = Case(m1, m2, 5, 8, put=True, div=div, N_i=N_MIX, dt_i=DT_MIX)
    U, _ = case.run(solver)
    field_check("mixed", U, case.ref())
    one = Case(m1, m2, 1, 8, law=tuple(x[:1] for x in case.law), put=True, div=div, N_i=N_MIX[:1], dt_i=DT_MIX[:1])
    assert one.strikes[0] == case.strikes[0]
    with tuned(solver, {"team_launch": 0}):
        assert np.array_equal(one.run(solver)[0][0], U[0])


def test_the_measured_shape_512x256(solver):
    """One 512x256 x3 call of 4 steps with per-instance matrices."""
    case = Case(512, 256, 3, 4, law=laws(3))
    U, d = case.run(solver)
    assert d.endswith(JUMP_WORDS), d
    field_check("512x256", U, case.ref())


# ---- one matrix for the batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,n", [(50, 25, 6), (300, 12, 40)])
def test_shared_matrix(solver, m1, m2, n):
    """Every instance on instance 0's grid with one (mu_J, sigma_J) and its own intensity (every fifth: 0); with the larger batch
    several instances ride on one staged strip.  The result is that of the per-instance matrices, bit for bit."""
    law = (np.array([LAM[(k + 3) % 5] for k in range(n)]), MU[0], SIG[0])
    case = Case(m1, m2, n, 3, law=law, same=True)
    U, d = case.run(solver, shared_grid=True)
    V, _ = case.run(solver)
    assert np.array_equal(U, V) and d.endswith(JUMP_WORDS)
    rows = [0, 1, 2, n - 1]
    field_check("shared", U, case.ref(law=(law[0], np.full(n, MU[0]), np.full(n, SIG[0])), rows=rows), rows)
    assert np.array_equal(U[rows[0]], U[5]) and not np.array_equal(U[0], U[1])  # (same law, same grid: the same field)


def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_broken_shared_grid_promise(solver):
    case = Case(50, 25, 3, 3, law=(0.5, -0.1, 0.15))
    assert status(solver.bates_timestepping, *case.head(), case.U0.copy(), 0.5, -0.1, 0.15, shared_grid=True) == INVALID
    # per-instance (mu_J, sigma_J): one matrix each, and nothing is promised about the grids
    U, _ = case.run(solver, law=(0.5, np.full(3, -0.1), np.full(3, 0.15)), shared_grid=True)
    field_check("after the broken promise", U, case.ref(law=(np.full(3, 0.5), np.full(3, -0.1), np.full(3, 0.15))))


# ---- the launchers ------------------------------------------------------------------------------------------------------------------------
def test_three_entry_points_on_50x25_x7(solver):
    m1, m2, n, N, eps = 50, 25, 7, 6, 1e-6
    strikes, grids, U0 = batch(m1, m2, n, True)
    law = laws(n)
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)]
    v0s = [v0s[k % len(v0s)] for k in range(n)]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    refkw = dict(put_strikes=strikes, V_0_i=v0s)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0) + law
    prices = solver.compute_base_prices_bates(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n, grids, ws,
                                              *law, per_instance=per)
    assert solver.describe_last_sweep().endswith(JUMP_WORDS)
    J, base = solver.compute_jacobian_bates(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n, grids,
                                            U0.copy(), *law, eps=eps, per_instance=per)
    assert solver.describe_last_sweep().endswith(JUMP_WORDS)
    po, Fo = JR.base_prices(*args, **refkw)
    Jo, bo = JR.jacobian(*args, eps=eps, **refkw)
    rel = np.abs(prices - po) / np.maximum(1.0, np.abs(po))
    print("launchers: prices %.2e relative, J %.2e" % (rel.max(), np.abs(J - Jo).max()))
    field_check("launcher field", ws.U, Fo)
    assert rel.max() <= 1e-10 and (np.abs(base - bo) / np.maximum(1.0, np.abs(bo))).max() <= 1e-10
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


class RefSolver:
    """The two Bates launchers on tests/jumps_ref.py, for the LM loop."""

    def _a(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U, law):
        return (m1, m2, N, dt, theta, r_d, r_f, rho, sigma, kappa, eta, S_0, V_0, grids.Vec_s, grids.Delta_s, np.asarray(U)) + tuple(law)

    def compute_jacobian_bates(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, U_0, lam, mu,
                               sig, shared_grid=False, eps=1e-6, **kw):
        return JR.jacobian(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, U_0, (lam, mu, sig)), eps=eps)

    def compute_base_prices_bates(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt, n, grids, ws, lam, mu,
                                  sig, shared_grid=False, **kw):
        return JR.base_prices(*self._a(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, N, theta, dt, grids, ws.U, (lam, mu, sig)))[0]


def test_calibrate_bates_two_iterations(solver):
    """The LM loop over the Bates launchers against the same loop driven by the reference: same iterates to the launchers' bounds
    (the bound and its reasoning: tests/test_gpu_bermudan.py)."""
    m1, m2, n, N = 50, 25, 4, 8
    strikes, grids, U0 = batch(m1, m2, n, False)
    law = (0.5, -0.10, 0.15)
    start = (Cm.KAPPA * 1.1, Cm.ETA * 0.9, Cm.SIGMA * 1.1, Cm.RHO * 0.9, Cm.V_0)
    market = JR.base_prices(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, *law)[0]
    out = {}
    for name, sv in (("gpu", solver), ("ref", RefSolver())):
        out[name] = H.calibrate_bates(sv, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, *start, m1, m2, N, Cm.THETA, grids, U0.copy(), market, *law,
                                      max_iter=2, tol=1e-12)
    assert "Bates" in solver.describe_last_sweep()
    a, b = out["gpu"], out["ref"]
    assert a["iterations"] == b["iterations"] == 2
    for key in ("kappa", "eta", "sigma", "rho", "v0"):
        assert abs(a[key] - b[key]) <= 1e-6, (key, a[key], b[key])
    assert np.abs(a["model_prices"] - b["model_prices"]).max() <= 1e-6


# ---- the graph cache and handle reuse ------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_first_capture_bit_for_bit(solver):
    case = Case(100, 12, 3, 6, put=True)
    with tuned(solver, {"graph": 1}):
        case.run(solver)  # (the buffers this shape needs are grown: growing one would empty the cache)
        c0 = Cm.graph_counts(solver)
        A, dA = case.run(solver)
        B, dB = case.run(solver)
        delta = Cm.graph_delta(c0, Cm.graph_counts(solver))
    assert delta["replays"] >= 1 and delta["captures"] <= 1 and dA == dB, delta
    assert np.array_equal(A, B)
    with tuned(solver, {"graph": 0}):
        E, _ = case.run(solver)
    assert np.array_equal(A, E)
    field_check("replayed", B, case.ref())


def test_two_laws_then_a_larger_batch_on_one_handle():
    """Different (mu_J, sigma_J) on the same batch replay the same loop over matrices built again; a larger batch then grows the
    buffers, which empties the cache: nothing is replayed over a moved buffer.  Each result is its own reference's."""
    with H.HestonADI(0) as sv:
        small = Case(100, 12, 3, 5)
        lawA, lawB = laws(3), laws(3, first=2)
        UA, _ = small.run(sv, law=lawA)
        c0 = Cm.graph_counts(sv)
        UB, _ = small.run(sv, law=lawB)
        UA2, _ = small.run(sv, law=lawA)
        d1 = Cm.graph_delta(c0, Cm.graph_counts(sv))
        big = Case(100, 12, 9, 5)
        UC, _ = big.run(sv)
        d2 = Cm.graph_delta(c0, Cm.graph_counts(sv))
        UA3, _ = small.run(sv, law=lawA)
    assert d1["replays"] == 2 and d1["captures"] == 0, d1
    assert d2["drops"] >= 1 and d2["captures"] >= 1, d2
    field_check("law A", UA, small.ref(law=lawA))
    field_check("law B", UB, small.ref(law=lawB))
    field_check("larger batch", UC, big.ref())
    assert np.array_equal(UA, UA2) and np.array_equal(UA, UA3) and not np.array_equal(UA, UB)


# ---- identity and refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{}, {"small_seq": 1, "small_pairs": 1}, {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}],
                         ids=["default", "seq2", "streaming"])
@pytest.mark.parametrize("m1,m2,scheme,theta", [(50, 25, 0, Cm.THETA), (100, 30, 0, Cm.THETA), (50, 25, H.SCHEME_MCS, TH_MCS)],
                         ids=["50x25", "100x30", "50x25-MCS"])
def test_zero_intensity_is_DO_timestepping_bit_for_bit(solver, tuning, m1, m2, scheme, theta):
    """Including the route and its words: every route stays open."""
    case = Case(m1, m2, 3, 5, scheme=scheme, theta=theta)
    with tuned(solver, tuning):
        V, d0 = case.plain(solver)
        U, d = case.run(solver, law=(0.0, -0.1, 0.15))
        assert d == d0 and "Bates" not in d, d
        assert np.array_equal(U, V)
        W, d2 = case.run(solver, law=(np.zeros(3), np.array(MU[:3]), np.array(SIG[:3])), shared_grid=True)
        assert np.array_equal(W, V) and d2 == d0


def test_refusals(solver):
    case = Case(50, 25, 3, 6)
    bt, head, U0 = solver.bates_timestepping, case.head(), case.U0
    nan3, inf3 = np.array([np.nan, 1.0, 1.0]), np.array([0.1, np.inf, 0.1])
    for bad in ((-0.5, -0.1, 0.15), (0.5, -0.1, 0.0), (0.5, -0.1, -0.2), (np.nan, -0.1, 0.15), (0.5, np.inf, 0.15), (0.5, -0.1, np.nan),
                (nan3, -0.1, 0.15), (0.5, nan3, 0.15), (0.5, -0.1, inf3), (np.array([0.5, -1e-9, 0.5]), -0.1, 0.15),
                (0.5, -0.1, np.array([0.1, 0.0, 0.1])),
                (6.5, -0.1, 0.15)):  # lambda dt = 6.5 / 6 > 1
        assert status(bt, *head, U0.copy(), *bad) == INVALID, bad
    bt(*head, U0.copy(), 6.0, -0.1, 0.15)  # lambda dt = 1 is admitted
    # ... per instance: instance 1 has dt = 1 / 4
    per = {"N_i": [6, 4, 5], "delta_t_i": [Cm.T / 6, Cm.T / 4, Cm.T / 5]}
    assert status(bt, *head, U0.copy(), 4.5, -0.1, 0.15, per_instance=per) == INVALID
    bt(*head, U0.copy(), np.array([4.5, 3.5, 4.5]), -0.1, 0.15, per_instance=per)
    for variant in (H.AM, H.AM_DIV):
        assert status(bt, *head, U0.copy(), 0.5, -0.1, 0.15, variant=variant, dividends=H.Dividends(*Cm.DIVS)) == UNSUPPORTED
    # grids that take the sequential passes
    for m1, m2 in ((1100, 30), (40, 600)):
        seq = Case(m1, m2, 1, 2, law=(0.5, -0.1, 0.15))
        assert status(seq.run, solver) == UNSUPPORTED
        Z, dz = seq.run(solver, law=(0.0, -0.1, 0.15))  # (zero intensity: the plain call, every route open)
        assert np.array_equal(Z, seq.plain(solver)[0])
    # what check_problem refuses keeps its status: a scheme with dividends
    assert status(bt, *head, U0.copy(), 0.5, -0.1, 0.15, variant=H.DIV, dividends=H.Dividends(*Cm.DIVS), scheme=H.SCHEME_MCS) == UNSUPPORTED
    # the raw ABI: a NULL struct, the fp32 state, NULL outputs
    lib, h = solver._lib, solver._h
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())
    good, keep = solver._jumps(3, 0.5, -0.1, 0.15, False)
    assert lib.hadi_bates_timestepping(h, C.byref(p), None) == INVALID
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_bates_timestepping(h, C.byref(p32), C.byref(good)) == UNSUPPORTED
    pv = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_base_prices_bates(h, C.byref(pv), Cm.S_0, Cm.V_0, C.byref(good), None) == INVALID
    out = np.zeros(3)
    assert lib.hadi_compute_base_prices_bates(h, C.byref(pv), Cm.S_0, Cm.V_0, None, C.c_void_p(out.ctypes.data)) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_jacobian_bates(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, C.byref(good), None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_jacobian_bates(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, None, None, None) == INVALID
    vs = np.ascontiguousarray(case.grids.Vec_s[0])
    G = np.zeros((51, 51))
    assert lib.hadi_debug_jump_matrix(h, 50, vs.ctypes.data_as(nat._dp), -0.1, 0.0, G.ctypes.data_as(nat._dp)) == INVALID
    assert lib.hadi_debug_jump_matrix(h, 50, None, -0.1, 0.15, G.ctypes.data_as(nat._dp)) == INVALID
    assert lib.hadi_version() == 2
    # and the handle still works
    assert lib.hadi_bates_timestepping(h, C.byref(p), C.byref(good)) == 0
    field_check("after the refusals", case.run(solver)[0], case.ref())


# ---- the recorded routes --------------------------------------------------------------------------------------------------------------------
def test_recorded_routes(solver):
    """tests/golden/route_selection_jumps.json: the device describes every recorded batch as it did when the file was recorded."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_jumps_routes as R
    fix = json.load(open(R.FIXTURE))
    if solver.device_info()["compute_units"] != fix["cu_count"]:
        pytest.fail("the fixture was recorded on %d compute units" % fix["cu_count"])
    for case, row in zip(R.CASES, fix["cases"]):
        if row["n"] > 300 and row["m1"] > 100:
            continue  # (the 512x256 x320 batch: the emulator test holds its words; 1.4 GB of state is not a few seconds)
        d0, d1 = R.describe(solver, H, np, case)
        assert (d0, d1) == (row["plain"], row["bates"]), row["name"]
