"""The resident sweep (hadi_sweep_resident: both passes of every Douglas step in one launch, one block per instance) against the
CPU oracle and against the streaming kernels it replaces, on the batch shapes where the plan picks it."""
import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm

pytestmark = pytest.mark.gpu

RESIDENT = "hadi_sweep_resident<8>"
R_F = 0.01  # (the strip kernels need r_d != r_f)


def _solve(solver, m1, m2, N, n, mode, per_instance=None, T=Cm.T):
    strikes = Cm.strikes_for(n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.call_payoff(strikes)
    U = U0.copy()
    solver.set_tuning("resident_sweep", mode)
    try:
        solver.DO_timestepping(m1, m2, N, T / N, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               per_instance=per_instance)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("resident_sweep", -1)
    return grids, U0, U, d


def _check_oracle(m1, m2, grids, U0, U, rows, Ns, dts, rtol=1e-10):
    for k in rows:
        p = O.make_params(m1, m2, Ns[k], dts[k], Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
        Uo, _, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k])
        err = np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        assert err <= rtol, "instance %d: field error %.3e" % (k, err)


def test_config2_batch_every_instance_against_the_oracle(solver):
    """256 European calls of 512x256, 20 steps: the plan's one-block strips in one round -- the resident launch by default.
    Every instance against the oracle, and the whole field against the streaming kernels (the same bodies: bit for bit so
    far; the bound is 1e-13 relative, the observed maximum is printed)."""
    m1, m2, N, n = 512, 256, 20, 256
    grids, U0, U, d = _solve(solver, m1, m2, N, n, -1)
    assert RESIDENT in d and "hadi_pass_a_strip<8,EU> (strips of 33 rows)" in d and "hadi_pass_b<8,EU>" in d, d
    _, _, Us, ds = _solve(solver, m1, m2, N, n, 0)
    assert RESIDENT not in ds, ds
    assert d.split(";")[:2] == ds.split(";")[:2]  # (the same row and column bodies are named)
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13
    assert np.isfinite(U).all()
    _check_oracle(m1, m2, grids, U0, U, range(n), [N] * n, [Cm.T / N] * n)


@pytest.mark.parametrize("n,want", [(512, "2 sub-batches of 256 instances"), (320, "2 sub-batches of 256 64 instances")])
def test_several_sub_batches(solver, n, want):
    """512 instances: two sub-batches of one round, each resident; 320: a resident round and a streaming remainder of 64
    (its row pass is three blocks per instance)."""
    m1, m2, N = 512, 256, 6
    grids, U0, U, d = _solve(solver, m1, m2, N, n, -1)
    assert RESIDENT in d and want in d, d
    if n == 320:
        assert "the others streaming" in d, d
    _, _, Us, ds = _solve(solver, m1, m2, N, n, 0)
    assert RESIDENT not in ds
    assert np.abs(U - Us).max() <= 1e-13 * np.abs(Us).max()
    _check_oracle(m1, m2, grids, U0, U, [0, 255, n - 1], [N] * n, [Cm.T / N] * n)


def test_per_instance_maturities(solver):
    """Each block loops to its own N: a batch of 256 with seven different (N_i, dt_i) against the streaming kernels and the
    oracle."""
    m1, m2, n = 512, 256, 256
    Ns = [4 + (k % 7) for k in range(n)]
    Ts = [0.25 + 0.1 * (k % 5) for k in range(n)]
    dts = [t / s for t, s in zip(Ts, Ns)]
    per = {"N_i": Ns, "delta_t_i": dts}
    grids, U0, U, d = _solve(solver, m1, m2, 1, n, -1, per_instance=per, T=1.0)
    assert RESIDENT in d, d
    _, _, Us, _ = _solve(solver, m1, m2, 1, n, 0, per_instance=per, T=1.0)
    assert np.abs(U - Us).max() <= 1e-13 * np.abs(Us).max()
    _check_oracle(m1, m2, grids, U0, U, range(0, n, 37), Ns, dts)


def test_tuning_key_and_eligibility(solver):
    assert solver.get_tuning("resident_sweep") == -1
    m1, m2, N = 512, 256, 3
    # pinned streaming geometry: the streaming kernels unless the resident sweep is forced
    solver.set_tuning("strip", 1)
    try:
        _, _, _, d = _solve(solver, m1, m2, N, 256, -1)
        assert RESIDENT not in d, d
        _, _, _, d = _solve(solver, m1, m2, N, 256, 1)
        assert RESIDENT in d, d
    finally:
        solver.set_tuning("strip", -1)
    # 160 instances leave 37 % of the CUs idle: two streams of strips, not the resident launch, even when forced
    _, _, _, d = _solve(solver, m1, m2, N, 160, 1)
    assert RESIDENT not in d and "two streams" in d, d
    # a cost-model constant that sends the plan to the shared ring
    solver.set_tuning("model_strip_row_ns", 10 ** 6)
    try:
        _, _, _, d = _solve(solver, m1, m2, N, 256, -1)
        assert RESIDENT not in d and "hadi_pass_a<8,1" in d, d
    finally:
        solver.set_tuning("model_strip_row_ns", 2800)


def test_handle_reuse_resident_streaming_resident(solver):
    """A / B / A on one handle: the resident launch, the streaming kernels (graph replay of the same buffers), the resident
    launch again -- all three the same field."""
    m1, m2, N, n = 512, 256, 4, 256
    _, _, Ua, da = _solve(solver, m1, m2, N, n, 1)
    _, _, Ub, db = _solve(solver, m1, m2, N, n, 0)
    _, _, Uc, dc = _solve(solver, m1, m2, N, n, 1)
    assert RESIDENT in da and RESIDENT not in db and da == dc
    assert np.array_equal(Ua, Uc)
    assert np.abs(Ua - Ub).max() <= 1e-13 * np.abs(Ub).max()


def test_profiling_runs_the_passes_as_separate_launches(solver):
    """Per-pass times need a kernel per pass: with profiling on, the sweep runs on the streaming kernels and reports them."""
    m1, m2, N, n = 512, 256, 5, 256
    solver.set_profiling(True)
    try:
        _, _, U, d = _solve(solver, m1, m2, N, n, -1)
        tm = solver.timing()
    finally:
        solver.set_profiling(False)
    assert RESIDENT not in d, d
    assert tm["pass_a_launches"] == N and tm["pass_b_launches"] == N
    assert 0 < tm["pass_a_ms"] and 0 < tm["pass_b_ms"] <= 1.05 * tm["sweep_ms"]


@pytest.mark.parametrize("m1,m2,n", [(512, 256, 64), (512, 256, 192), (1024, 512, 16), (256, 128, 512)])
def test_other_batch_shapes_stay_streaming(solver, m1, m2, n):
    """Batches the plan runs as several strip blocks per instance (64), with a partial round (192: two streams), paired strips
    (1024x512) or 4 nodes per lane (256x128) keep the streaming kernels."""
    _, _, U, d = _solve(solver, m1, m2, 1, n, -1)
    assert RESIDENT not in d, d
    assert np.isfinite(U).all()


def test_debug_hooks_keep_the_streaming_kernels(solver):
    """The column-pass timing hook (debug_fault 256) belongs to the streaming kernels: with it set the resident launch is not
    used (its idle wavefronts would keep a barrier schedule the hooked solve skips)."""
    solver.set_tuning("debug_fault", 256)
    try:
        _, _, _, d = _solve(solver, 512, 256, 1, 256, 1)
    finally:
        solver.set_tuning("debug_fault", 0)
    assert RESIDENT not in d, d
