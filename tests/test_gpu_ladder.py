"""The maturity ladder on the device (hadi_maturity_ladder, hadi_compute_base_prices_ladder, hadi_compute_jacobian_ladder): one
case per execution path, each with its tuning keys pinned so that the ladder call and the single calls run the same kernels.
Every snapshot must equal the single call with N = snap_steps[q] on the same handle BIT FOR BIT (the ladder's definition) and
lie within 1e-10 max|U_ref| of the oracle at that N (well-conditioned grids, asserted).  Calls run at the canonical r_f = 0:
with r_f != 0 the call's boundary tables depend on N and the library refuses the ladder (tests/test_oracle_ladder.py)."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle as O

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import common as Cm
import scheme_ref as S

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
VAR = {"EU": H.EU, "AM": H.AM, "DIV": H.DIV, "AM_DIV": H.AM_DIV}
DEFAULTS = {"small_grid": 1, "small_seq": -1, "small_pairs": -1, "small_sch": -1, "american_p": 1, "streams": 0, "strip": -1,
            "resident_sweep": -1, "team_launch": -1, "graph": 1}
LADDER = "maturity ladder"


@contextlib.contextmanager
def tuned(sv, **kw):
    """The handle is shared by the session: every key goes back to its default."""
    for k, v in kw.items():
        sv.set_tuning(k, v)
    try:
        yield
    finally:
        for k in kw:
            sv.set_tuning(k, DEFAULTS[k])


_batches = {}


def _batch(m1, m2, n):
    if (m1, m2, n) not in _batches:
        strikes = Cm.well_conditioned_strikes(m1, n)
        grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
        Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
        _batches[(m1, m2, n)] = (strikes, grids)
    return _batches[(m1, m2, n)]


def _paying_steps(N, dt):
    """The dating rule of hadi.h on the canonical schedule."""
    out, idx, dates = [], 0, Cm.DIVS[0]
    for n in range(1, N + 1):
        if idx < len(dates) and n * dt <= dates[idx] < (n + 1) * dt:
            out.append(n)
        if idx < len(dates) and n * dt > dates[idx]:
            idx += 1
    return out


class Case:
    def __init__(self, m1, m2, n, N, variant="EU", scheme=0, theta=Cm.THETA, put=False, dts=None, r_f=Cm.R_F):
        self.m1, self.m2, self.n, self.N, self.variant, self.scheme, self.theta, self.put, self.r_f = m1, m2, n, N, variant, scheme, theta, put, r_f
        self.strikes, self.grids = _batch(m1, m2, n)
        self.U0 = Cm.put_payoff(self.grids.Vec_s, self.strikes, m2) if put else self.grids.call_payoff(self.strikes)
        self.div = H.Dividends(*Cm.DIVS) if "DIV" in variant else None
        self.dts = dts
        self.v0 = Cm.v0_for(m2)

    def kw(self):
        k = dict(variant=VAR[self.variant], dividends=self.div, scheme=self.scheme)
        if "AM" in self.variant:
            k["U_0"] = self.U0
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.dts:
            k["per_instance"] = {"delta_t_i": self.dts}
        return k

    def head(self, N):
        return (self.m1, self.m2, N, Cm.T / self.N, self.theta, Cm.R_D, self.r_f) + MODEL + (self.grids,)

    def ladder(self, sv, snaps):
        out = sv.maturity_ladder(*self.head(self.N), self.U0.copy(), Cm.S_0, self.v0, snaps, **self.kw())
        return out, sv.describe_last_sweep()

    def node(self, k):
        i0 = O.find_s_index(self.grids.Vec_s[k], Cm.S_0)
        j0 = O.find_v_index(self.grids.Vec_v[k], self.v0)
        assert i0 >= 0
        return i0 + j0 * (self.m1 + 1)

    def single(self, sv, N):
        """The single-maturity call: the N-step sweep, the node read off its field."""
        U = self.U0.copy()
        sv.DO_timestepping(*self.head(N), U, **self.kw())
        return np.array([U[k, self.node(k)] for k in range(self.n)]), sv.describe_last_sweep()

    def oracle(self, N):
        g = self.grids
        out, scale = np.empty(self.n), np.empty(self.n)
        for k in range(self.n):
            dt = self.dts[k] if self.dts else Cm.T / self.N
            if self.scheme:
                p = O.make_params(self.m1, self.m2, N, dt, self.theta, Cm.R_D, self.r_f, *MODEL, O.EU)
                U = S.solve_one(p, g.Vec_s[k], g.Vec_v[k], g.Delta_s[k], g.Delta_v[k], self.U0[k], self.scheme)
            else:
                p = O.make_params(self.m1, self.m2, N, dt, self.theta, Cm.R_D, self.r_f, *MODEL, Cm.VARIANT[self.variant],
                                  Cm.DIVS if self.div else None, option_type=O.PUT if self.put else O.CALL,
                                  strikes=self.strikes[k] if self.put else None)
                U = O.solve(p, g.Vec_s[k], g.Vec_v[k], g.Delta_s[k], g.Delta_v[k], self.U0[k],
                            self.U0[k] if "AM" in self.variant else None)[0]
            out[k], scale[k] = U[self.node(k)], np.abs(U).max()
        return out, scale


def _check(sv, case, snaps, tuning, names, bits=True):
    """names: what the description of the ladder call AND of the single calls must contain (the same kernels)."""
    with tuned(sv, **tuning):
        out, d = case.ladder(sv, snaps)
        assert out.shape == (case.n, len(snaps))
        assert LADDER in d and all(x in d for x in names), d
        worst = 0.0
        for q, N in enumerate(snaps):
            one, d1 = case.single(sv, N)
            assert LADDER not in d1 and all(x in d1 for x in names), d1
            if bits:
                assert np.array_equal(out[:, q], one), (N, out[:, q] - one)
            ref, scale = case.oracle(N)
            err = np.abs(out[:, q] - ref) / scale
            worst = max(worst, err.max())
            assert (err <= 1e-10).all(), (N, err)
        print("%s | snaps %s: worst |diff| / max|U_ref| vs oracle %.2e" % (d[:60], list(snaps), worst))
    return out


# ---- the whole-loop kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["EU", "AM"])
def test_block_kernel(solver, variant):
    _check(solver, Case(50, 25, 3, 8, variant), [1, 4, 5, 8], {"small_seq": 0}, ["hadi_small_kernel<"])


def test_sequential_kernel(solver):
    _check(solver, Case(50, 25, 3, 8), [2, 5, 7], {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<"])
    _check(solver, Case(65, 16, 2, 5), [1, 2, 3, 4, 5], {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<2>"])


def test_pairs_kernel_with_an_odd_last_instance(solver):
    _check(solver, Case(50, 25, 3, 8), [1, 8], {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<"])


@pytest.mark.parametrize("scheme,theta,name", [(H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")], ids=["MCS", "HV"])
def test_scheme_kernel(solver, scheme, theta, name):
    _check(solver, Case(50, 25, 3, 6, scheme=scheme, theta=theta), [1, 3, 6], {"small_sch": 1}, ["hadi_small_sch_kernel<1,%s>" % name])
    _check(solver, Case(128, 32, 2, 4, scheme=scheme, theta=theta), [2, 3], {"small_sch": 1}, ["hadi_small_sch_kernel<2,%s>" % name])


@pytest.mark.parametrize("variant", ["DIV", "AM_DIV"])
def test_dividends_with_a_snapshot_on_a_paying_step(solver, variant):
    N = 10
    pay = _paying_steps(N, Cm.T / N)
    assert len(pay) >= 2
    snaps = sorted(set([1, pay[0], pay[0] + 1, pay[1], N]))
    _check(solver, Case(50, 25, 3, N, variant), snaps, {"small_seq": 0}, ["hadi_small_kernel<"])
    if variant == "DIV":
        _check(solver, Case(50, 25, 3, N, variant), snaps, {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<"])
    _check(solver, Case(50, 25, 3, N, variant), snaps, {"small_grid": 0, "american_p": 0}, ["row pass"])


def test_puts(solver):
    _check(solver, Case(50, 25, 3, 6, put=True, r_f=0.007), [1, 3, 6], {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<"])
    _check(solver, Case(50, 25, 3, 6, "AM", put=True, r_f=0.007), [2, 6], {"small_seq": 0}, ["hadi_small_kernel<"])
    _check(solver, Case(100, 30, 2, 4, put=True, r_f=0.007), [1, 4], {"small_grid": 0}, ["row pass"])


def test_per_instance_delta_t(solver):
    c = Case(50, 25, 3, 6, dts=[Cm.T / 6, 0.5 / 6, 0.25 / 6])
    _check(solver, c, [2, 3, 6], {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<"])
    _check(solver, c, [2, 6], {"small_grid": 0}, ["row pass"])


# ---- the streaming kernels ----------------------------------------------------------------------------------------------------
# (one node per lane -- 50x25 -- has no strip kernel: "strip" = 1 leaves it on the shared ring)
@pytest.mark.parametrize("m1,m2,strip,name", [(50, 25, 0, "hadi_pass_a<"), (50, 25, 1, "hadi_pass_a<"), (100, 30, 0, "hadi_pass_a<"),
                                              (100, 30, 1, "hadi_pass_a_strip<")],
                         ids=["50x25-ring", "50x25-strip-key", "100x30-ring", "100x30-strips"])
def test_streaming(solver, m1, m2, strip, name):
    _check(solver, Case(m1, m2, 3, 6), [1, 4, 6], {"small_grid": 0, "strip": strip}, [name, "row pass"])


def test_streaming_scheme(solver):
    _check(solver, Case(50, 25, 3, 5, scheme=H.SCHEME_MCS, theta=TH_MCS), [1, 2, 5], {"small_grid": 0, "small_sch": 0}, ["row pass", "MCS"])


def test_two_streams(solver):
    _check(solver, Case(50, 25, 4, 6), [2, 5, 6], {"small_grid": 0, "streams": 2}, ["side by side on two streams"])


def test_american_streaming_explicit_pair(solver):
    _check(solver, Case(50, 25, 3, 6, "AM"), [1, 3, 6], {"small_grid": 0, "american_p": 0}, ["row pass"])


def test_american_streaming_against_the_p_representation(solver):
    """"american_p" = 1: the single call keeps P, the ladder call the explicit pair -- the oracle bound only."""
    case, snaps = Case(50, 25, 3, 6, "AM"), [1, 3, 6]
    with tuned(solver, small_grid=0, american_p=1):
        out, d = case.ladder(solver, snaps)
        assert LADDER in d and "no lambda_bar array" not in d, d
        _, d1 = case.single(solver, 6)
        assert "no lambda_bar array" in d1, d1
        for q, N in enumerate(snaps):
            ref, scale = case.oracle(N)
            assert (np.abs(out[:, q] - ref) <= 1e-10 * scale).all(), N


# ---- exclusions ---------------------------------------------------------------------------------------------------------------
def _excluded(sv, case, snaps, tuning, kernel):
    with tuned(sv, **tuning):
        _, d1 = case.single(sv, case.N)
        assert kernel in d1, d1
        out, d = case.ladder(sv, snaps)
        assert kernel not in d and LADDER in d and "row pass" in d, d
        g = case.grids
        for q, N in enumerate(snaps):
            p = O.make_params(case.m1, case.m2, N, Cm.T / case.N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, O.EU)
            Uo = O.solve_batch(p, g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, case.U0)[0]
            ref = np.array([Uo[k, case.node(k)] for k in range(case.n)])
            assert (np.abs(out[:, q] - ref) <= 1e-10 * np.abs(Uo).max(axis=1)).all(), N


def test_never_the_resident_sweep(solver):
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the resident sweep's one round of 256 instances needs the 256-CU device")
    # ("strip" = 1: at 264x8 the plan's own choice is the shared ring, and the resident sweep is the strips' body)
    _excluded(solver, Case(264, 8, 256, 4), [2, 4], {"resident_sweep": 1, "strip": 1}, "hadi_sweep_resident")


def test_never_the_team_launch(solver):
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the team launch needs the 256-CU device")
    _excluded(solver, Case(200, 16, 2, 4), [1, 4], {"team_launch": 1}, "hadi_team_kernel")


# ---- graph cache --------------------------------------------------------------------------------------------------------------
def test_graph_capture_replay_and_key(solver):
    case = Case(50, 25, 3, 6)
    with tuned(solver, small_grid=0, graph=1):
        plain0, _ = case.single(solver, 6)
        c0 = Cm.graph_counts(solver)
        a, _ = case.ladder(solver, [2, 4, 6])
        c1 = Cm.graph_counts(solver)
        b, _ = case.ladder(solver, [2, 4, 6])
        c2 = Cm.graph_counts(solver)
        # (the session's handle may arrive with a full cache: an eviction on capture is not this test's business)
        d01, d12 = Cm.graph_delta(c0, c1), Cm.graph_delta(c1, c2)
        assert (d01["captures"], d01["replays"]) == (1, 0), d01
        assert (d12["captures"], d12["replays"], d12["drops"], d12["evictions"]) == (0, 1, 0, 0), d12
        assert np.array_equal(a, b)
        other, _ = case.ladder(solver, [1, 3, 5])  # same length, other steps: a new loop, the new steps' values
        c3 = Cm.graph_counts(solver)
        assert Cm.graph_delta(c2, c3)["captures"] == 1 and Cm.graph_delta(c2, c3)["replays"] == 0
        for q, N in enumerate([1, 3, 5]):
            assert np.array_equal(other[:, q], case.single(solver, N)[0])
        assert not np.array_equal(other, a)
        plain1, _ = case.single(solver, 6)  # a plain solve afterwards: its own loop, its own bits
        assert np.array_equal(plain0, plain1) and np.array_equal(plain1, a[:, 2])


# ---- the launchers ------------------------------------------------------------------------------------------------------------
def test_base_prices_ladder_with_per_instance_v0(solver):
    m1, m2, n, N = 50, 25, 4, 8
    strikes, grids = _batch(m1, m2, n)
    U0 = grids.call_payoff(strikes)
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s}
    snaps = [1, 5, 8]
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1))
    for tuning, name in (({"small_seq": 0}, "hadi_small_kernel<"), ({"small_grid": 0}, "row pass")):
        with tuned(solver, **tuning):
            ws.U[...] = U0
            out = solver.compute_base_prices_ladder(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), N, Cm.THETA,
                                                    Cm.T / N, n, grids, ws, snaps, per_instance=per)
            assert name in solver.describe_last_sweep() and LADDER in solver.describe_last_sweep()
            assert np.array_equal(ws.U, U0)  # not written
            for q, Nq in enumerate(snaps):
                ws.U[...] = U0
                one = solver.compute_base_prices(Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, Cm.R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), Nq,
                                                 Cm.THETA, Cm.T / N, n, grids, ws, per_instance=per)
                assert np.array_equal(out[:, q], one), (name, Nq)
            ws.U[...] = U0


def _jac_setup():
    j = Cm.GOLDEN["jacobian"]
    strikes = [float(k) for k in j["strikes"]]
    grids = H.GridViewsBatch.for_strikes(j["m1"], j["m2"], Cm.S_0, Cm.V_0, strikes)
    return j, strikes, grids, grids.call_payoff(strikes)


@pytest.mark.parametrize("variant", ["EU", "AM_DIV"])
def test_jacobian_ladder_on_a_whole_loop_path_bit_for_bit(solver, variant):
    j, strikes, grids, U0 = _jac_setup()
    m1, m2, N, n = j["m1"], j["m2"], j["N"], len(strikes)
    snaps = [5, 12, 20]
    div = H.Dividends(*Cm.DIVS) if variant == "AM_DIV" else None
    tuning = {"small_seq": 0} if variant == "AM_DIV" else {"small_seq": 1, "small_pairs": 1}
    with tuned(solver, **tuning):
        J, base = solver.compute_jacobian_ladder(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), N, Cm.THETA,
                                                 Cm.T / N, n, grids, U0, snaps, eps=j["eps"], variant=VAR[variant], dividends=div)
        d = solver.describe_last_sweep()
        assert J.shape == (n, 3, 5) and base.shape == (n, 3) and LADDER in d and "whole time loop" in d, d
        for q, Nq in enumerate(snaps):
            args = (Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, Cm.R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), Nq, Cm.THETA, Cm.T / N, n, grids, U0)
            J1, b1 = solver.compute_jacobian(*args, eps=j["eps"]) if variant == "EU" else \
                solver.compute_jacobian_american_dividends(*args, div, eps=j["eps"])
            assert np.array_equal(J[:, q, :], J1) and np.array_equal(base[:, q], b1), Nq


def test_jacobian_ladder_on_the_streaming_path_vs_oracle(solver):
    """The tolerances of test_gpu_parity.py::test_jacobian_vs_oracle: prices 1e-9, J 2e-4 (2e-5 on the first three rows)."""
    j, strikes, grids, U0 = _jac_setup()
    m1, m2, N, n = j["m1"], j["m2"], j["N"], len(strikes)
    snaps = [5, 12, 20]
    with tuned(solver, small_grid=0):
        J, base = solver.compute_jacobian_ladder(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), N, Cm.THETA,
                                                 Cm.T / N, n, grids, U0, snaps, eps=j["eps"])
        assert "row pass" in solver.describe_last_sweep() and LADDER in solver.describe_last_sweep()
    for q, Nq in enumerate(snaps):
        p = O.make_params(m1, m2, Nq, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, O.EU)
        Jo, baseo = O.jacobian(p, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, eps=j["eps"])
        assert np.abs(base[:, q] - baseo).max() <= 1e-9
        assert np.abs(J[:, q, :] - Jo).max() <= 2e-4 and np.abs(J[:3, q, :] - Jo[:3]).max() <= 2e-5, Nq
    assert abs(base[0, 2] - j["base_price_0"]) <= 1e-9  # the row the reference printed, at the ladder's top


def test_device_memory_outputs(solver):
    import torch
    case = Case(50, 25, 3, 6)
    host, _ = case.ladder(solver, [2, 6])
    dev = torch.device("cuda", 0)
    g = case.grids.to(dev)
    U = torch.from_numpy(case.U0.copy()).to(dev)
    out = solver.maturity_ladder(*case.head(6)[:-1], g, U, Cm.S_0, case.v0, [2, 6])
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), host)
    assert np.array_equal(U.cpu().numpy(), case.U0)


# ---- errors -------------------------------------------------------------------------------------------------------------------
def _status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_errors(solver):
    INVALID, UNSUPPORTED, NOT_ON_GRID = 1, 2, 4
    case = Case(50, 25, 3, 6)
    head, U0 = case.head(6), case.U0
    lad = solver.maturity_ladder
    for bad in ([0, 3], [3, 3], [4, 2], [7], [1, 2, 3, 4, 5, 6, 7], [-1]):
        assert _status(lad, *head, U0.copy(), Cm.S_0, case.v0, bad) == INVALID, bad
    assert _status(lad, *head, U0.copy(), Cm.S_0, case.v0, [2], per_instance={"N_i": [6, 6, 6]}) == INVALID
    assert _status(lad, *head, U0.copy(), Cm.S_0, case.v0, [2], per_instance={"V_0_i": [0.04] * 3}) == INVALID  # (as hadi_compute_greeks)
    assert _status(lad, *head, U0.copy(), Cm.S_0 + 0.123, case.v0, [2]) == NOT_ON_GRID
    assert lad(*head, U0.copy(), Cm.S_0, 0.0123456, [2]).shape == (3, 1)  # V_0 off the grid: v-row 0, as the price pick
    assert _status(lad, *head, U0.copy(), Cm.S_0, case.v0, [2], variant=H.AM, U_0=U0, scheme=H.SCHEME_MCS) == UNSUPPORTED
    # call boundary data with r_f != 0: the tables depend on N
    h7 = head[:6] + (0.007,) + head[7:]
    assert _status(lad, *h7, U0.copy(), Cm.S_0, case.v0, [2]) == UNSUPPORTED
    # the raw ABI: NULL outputs, NULL steps, the fp32 state
    steps = np.array([2, 6], dtype=np.int32)
    sp = steps.ctypes.data_as(C.POINTER(C.c_int))
    out = np.zeros((3, 2))
    Jb = np.zeros((3, 2, 5))
    lib, h = solver._lib, solver._h
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())
    assert lib.hadi_maturity_ladder(h, C.byref(p), Cm.S_0, case.v0, 2, sp, None) == INVALID
    assert lib.hadi_maturity_ladder(h, C.byref(p), Cm.S_0, case.v0, 2, None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_maturity_ladder(h, C.byref(p), Cm.S_0, case.v0, 0, sp, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_base_prices_ladder(h, C.byref(p), Cm.S_0, case.v0, 2, sp, None) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_jacobian_ladder(h, C.byref(pj), Cm.S_0, case.v0, 1e-6, 2, sp, None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_jacobian_ladder(h, C.byref(pj), Cm.S_0, case.v0, 1e-6, 2, sp, C.c_void_p(Jb.ctypes.data), None) == INVALID
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_maturity_ladder(h, C.byref(p32), Cm.S_0, case.v0, 2, sp, C.c_void_p(out.ctypes.data)) == UNSUPPORTED
    # and the handle still works
    assert lib.hadi_maturity_ladder(h, C.byref(p), Cm.S_0, case.v0, 2, sp, C.c_void_p(out.ctypes.data)) == 0
    assert np.array_equal(out, case.ladder(solver, [2, 6])[0])
