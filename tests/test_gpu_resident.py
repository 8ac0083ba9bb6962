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


# ======================================================================================================================
# The admitted domain.  The plan runs hadi_sweep_resident<8> for 246 .. 256 European fp64 instances per sub-batch on every grid
# with 256 < m1 <= 512 and m2 <= 263 ("resident_sweep" = 1 with "strip" = 1 forces it on each of them); the tests above sit on
# one grid of that domain.  Every case below
#   * asserts from describe_last_sweep() that the resident kernel ran -- a case that fell back to the streaming kernels fails
#     instead of comparing them with themselves -- and which strip height / chunk count it ran on,
#   * runs the same call with "resident_sweep" = 0 and compares the two fields (<= 1e-13 max|U|; 0 observed: the same bodies),
#   * compares with the oracle at 1e-10 max|U| on grids that obey the 30x conditioning rule of DESIGN.md section 2 -- asserted
#     for every instance (Cm.assert_well_conditioned), never filtered: Cm.strikes_for(256) does NOT obey it.
# Oracle's own distance from the binary128 adjudicator (oracle.solve_xp), measured once per (shape, parameter set) on the CPU:
# see DESIGN.md section 2 ("resident sweep, admitted domain"); all below 1e-11, so the 1e-10 bound keeps its 10x margin.
# The batch-size edges assume the MI355X's 256 CUs (asserted where they matter).
# ======================================================================================================================
from concurrent.futures import ThreadPoolExecutor

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
SUBSET = lambda n: sorted({0, 1, 7, 8, n - 2, n - 1})  # the fixed subset of the larger cases (the XCD remap's first round and the ends)


@pytest.fixture(scope="module")
def strict_solver():
    """libhadi_strict.so: the same sources with every counted `s_waitcnt vmcnt(n)` replaced by a full drain."""
    import __graft_entry__ as G
    s = H.HestonADI(0, lib_path=G.build_libhadi_strict())
    yield s
    s.close()


def _inputs(m1, m2, n, put=False, strikes=None):
    """Well-conditioned batch: strikes from Cm.well_conditioned_strikes, V_0 from Cm.v0_for -- and the rule asserted."""
    strikes = Cm.well_conditioned_strikes(m1, n) if strikes is None else strikes
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    return strikes, grids, U0


def _run(sv, m1, m2, N, grids, U0, mode, strip=None, theta=Cm.THETA, r_f=R_F, model=MODEL, per=None, put_strikes=None, dt=None):
    U = U0.copy()
    sv.set_tuning("resident_sweep", mode)
    if strip is not None:
        sv.set_tuning("strip", strip)
    try:
        kw = {} if put_strikes is None else dict(option_type=H.PUT, strikes=put_strikes)
        sv.DO_timestepping(m1, m2, N, Cm.T / N if dt is None else dt, theta, Cm.R_D, r_f, *model, grids, U, per_instance=per, **kw)
        d = sv.describe_last_sweep()
    finally:
        sv.set_tuning("resident_sweep", -1)
        if strip is not None:
            sv.set_tuning("strip", -1)
    return U, d


def _resident_and_streaming(sv, m1, m2, N, grids, U0, want_resident=True, **kw):
    """The call with "resident_sweep" = 1 and again with 0 (same tuning otherwise); the resident kernel must have run in the
    first (want_resident) and must not have run in the second; the two fields to 1e-13."""
    U, d = _run(sv, m1, m2, N, grids, U0, 1, **kw)
    assert (RESIDENT in d) == want_resident, d
    Us, ds = _run(sv, m1, m2, N, grids, U0, 0, **kw)
    assert RESIDENT not in ds, ds
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("  resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13
    assert np.isfinite(U).all()
    return U, d, ds


def _oracle_check(m1, m2, grids, U0, U, rows, N=None, theta=Cm.THETA, r_f=R_F, model=MODEL, per=None, put_strikes=None, dt=None, threads=16):
    """Instances `rows` against the oracle: one solve_batch(threads=16) where the parameters are uniform, one solve per
    instance on 16 threads where they are not.  Prints the observed maximum, asserts 1e-10."""
    rows = list(rows)
    O.lib()
    if per is None:
        p = O.make_params(m1, m2, N, Cm.T / N if dt is None else dt, theta, Cm.R_D, r_f, *model, O.EU, option_type=O.CALL if put_strikes is None else O.PUT,
                          strikes=None if put_strikes is None else np.asarray(put_strikes, dtype=np.float64)[rows])
        Uo, _, _ = O.solve_batch(p, grids.Vec_s[rows], grids.Vec_v[rows], grids.Delta_s[rows], grids.Delta_v[rows], U0[rows],
                                 threads=threads)
        errs = np.abs(U[rows] - Uo).max(axis=1) / np.abs(Uo).max(axis=1)
    else:
        def one(k):
            mk = tuple(per[key][k] for key in ("rho_i", "sigma_i", "kappa_i", "eta_i"))
            p = O.make_params(m1, m2, per["N_i"][k], per["delta_t_i"][k], theta, Cm.R_D, r_f, *mk, O.EU)
            Uo, _, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k])
            return np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        with ThreadPoolExecutor(threads) as ex:
            errs = np.array(list(ex.map(one, rows)))
    print("  vs oracle, %d instances: max field error %.3e (instance %d)" % (len(rows), errs.max(), rows[int(errs.argmax())]))
    assert errs.max() <= 1e-10, "instance %d: field error %.3e" % (rows[int(errs.argmax())], errs.max())


# ---- A. shapes ------------------------------------------------------------------------------------------------------
SHAPES_A = [(400, m2) for m2 in (3, 9, 31, 32, 33, 56, 57, 64, 65, 66, 98, 131, 132, 164, 197, 230, 262, 263)] + \
           [(m1, m2) for m1 in (257, 448, 511, 512) for m2 in (100, 263)]


def test_shape_list_covers_the_chunk_counts_and_strip_edges():
    """What SHAPES_A is for, asserted on the list itself: P = 1 .. 8 column chunks with m2 + 1 = 33 k and 33 k + 1, a last
    strip of one row (m2 = 56), an empty last strip (m2 = 31, 32: 8 strips of 4 / 5 rows would be 32 / 40), wavefronts without a
    strip (m2 = 3), the plan's `rs >= 8` rule from both sides (56 / 57 rows), and the ends of the m1 range."""
    m2s = [m2 for m1, m2 in SHAPES_A if m1 == 400]
    assert sorted({(m2 + 33) // 33 for m2 in m2s}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert {k for k in range(1, 9) if 33 * k - 1 in m2s} == set(range(1, 9)) and {k for k in range(1, 8) if 33 * k in m2s} == {1, 2, 4}
    rows = lambda m2: [max(0, min((m2 + 8) // 8, m2 + 1 - w * ((m2 + 8) // 8))) for w in range(8)]
    assert rows(56) == [8] * 7 + [1] and rows(3) == [1] * 4 + [0] * 4 and rows(32)[-1] == 0 and rows(31)[-1] == 4 and rows(9)[-3:] == [0, 0, 0]
    assert (55 + 8) // 8 < 8 <= (56 + 8) // 8
    assert {m1 for m1, _ in SHAPES_A} == {257, 400, 448, 511, 512}


@pytest.mark.parametrize("m1,m2", SHAPES_A)
def test_shape_sweep(solver, m1, m2):
    """256 calls, 4 steps, forced ("resident_sweep" = 1, "strip" = 1): every instance against the oracle; the description must
    name the strip height ceil((m2 + 1) / 8) and the chunk count ceil((m2 + 1) / 33)."""
    n, N = 256, 4
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, ds = _resident_and_streaming(solver, m1, m2, N, grids, U0, strip=1)
    rs, P = (m2 + 8) // 8, (m2 + 33) // 33
    assert "hadi_pass_a_strip<8,EU> (strips of %d rows)" % rs in d and "hadi_pass_b<8,EU> (%d chunks of 33 rows" % P in d, d
    assert d.split(";")[:2] == ds.split(";")[:2]  # (the streaming run: the same row and column bodies at the same geometry)
    _oracle_check(m1, m2, grids, U0, U, range(n), N=N)


# ---- B. batch sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2", [(512, 256), (300, 80)])
@pytest.mark.parametrize("n", [245, 246, 247, 250, 255, 256])
def test_batch_sizes_around_the_idle_threshold(solver, m1, m2, n):
    """One block per instance in one round of CUs with less than HADI_TWO_STREAM_IDLE = 0.04 of them idle: on 256 CUs that is
    246 .. 256 instances (10 / 256 = 0.039 < 0.04 <= 11 / 256 = 0.043) -- padded grids of 248 and 256 blocks whose last XCD round
    has `inst >= n_inst` blocks.  245 instances must NOT be resident even when asked for (the streaming strips)."""
    assert solver.device_info()["compute_units"] == 256  # (the thresholds below are the 256-CU device's)
    assert 1 - 246 / 256 < 0.04 <= 1 - 245 / 256
    N = 3
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0, want_resident=n >= 246)
    if n < 246:
        assert "hadi_pass_a_strip<8,EU>" in d, d
        if m1 == 512:  # (two halves side by side; at 300x80 the plan of a half batch leaves the strips, so the batch stays whole)
            assert "2 sub-batches of 123 122 instances" in d and "side by side on two streams" in d, d
    else:
        assert "both passes of every step in one launch: " + RESIDENT in d and "sub-batches" not in d, d
    _oracle_check(m1, m2, grids, U0, U, range(n) if m1 == 300 else SUBSET(n), N=N)


@pytest.mark.parametrize("n,want,whole", [
    (502, "2 sub-batches of 256 246 instances (each with the geometry of its own size), side by side on two streams", True),
    (500, "3 sub-batches of 256 122 122 instances (each with the geometry of its own size), the last two side by side on two streams", False)])
def test_two_rounds_and_a_remainder(solver, n, want, whole):
    """512x256: 502 = 256 + 246 instances are two resident sub-batches; 500 = 256 + 244 are one resident round and a remainder
    that leaves 4.7 % of the CUs idle -- cut in two halves of 122 that run on the streaming kernels, side by side."""
    assert solver.device_info()["compute_units"] == 256
    m1, m2, N = 512, 256, 3
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0)
    assert want in d, d
    if whole:
        assert "both passes of every step in one launch: " + RESIDENT in d, d
    else:
        assert "for 1 sub-batches of one round: " + RESIDENT in d and "the others streaming" in d, d
    _oracle_check(m1, m2, grids, U0, U, sorted(set(SUBSET(n)) | {255, 256, 257}), N=N)


# ---- C. inputs ------------------------------------------------------------------------------------------------------
def _per_instance_draws(n):
    """256 distinct (rho, sigma, kappa, eta) from the ranges tools/gpu_sweep.py draws, seeded; maturities with N_i = 1 (instance
    0) next to the maximum (instance 1)."""
    rng = np.random.default_rng(20261)
    per = {"rho_i": rng.uniform(-0.95, 0.5, n), "sigma_i": rng.uniform(0.1, 0.8, n), "kappa_i": rng.uniform(0.3, 4.0, n),
           "eta_i": rng.uniform(0.01, 0.2, n)}
    Ns = [(1, 6, 2, 5, 3, 4)[k % 6] for k in range(n)]
    Ts = [0.25 + 0.1 * (k % 5) for k in range(n)]
    per["N_i"] = Ns
    per["delta_t_i"] = [t / s for t, s in zip(Ts, Ns)]
    assert len({tuple(per[key][k] for key in ("rho_i", "sigma_i", "kappa_i", "eta_i")) for k in range(n)}) == n
    assert Ns[0] == 1 and Ns[1] == max(Ns)
    return per


INPUTS_C = {  # name: (keyword arguments of the run, stays on the resident kernel)
    "per_instance": (dict(per=True), True),
    "put": (dict(put=True), True),
    "theta_0.5": (dict(theta=0.5), True),
    "theta_1": (dict(theta=1.0), True),          # (the strips' kap = (1 - theta) / theta is 0)
    "rho_0": (dict(model=(0.0,) + MODEL[1:]), True),
    "rho_-0.9": (dict(model=(-0.9,) + MODEL[1:]), True),
    "r_f_above_r_d": (dict(r_f=0.04), True),
    "r_f_equals_r_d": (dict(r_f=Cm.R_D), False),  # no strips without r_d - r_f: the shared ring, not the resident kernel
    # ... nor with theta = 0 (dt = 1e-6: the explicit scheme is only stable for tiny steps on these grids, as in
    # test_gpu_parity.py::test_strip_row_pass_theta_range)
    "theta_0": (dict(theta=0.0, dt=1e-6), False),
}


@pytest.mark.parametrize("m1,m2", [(300, 80), (512, 256)])
@pytest.mark.parametrize("name", list(INPUTS_C))
def test_inputs(solver, m1, m2, name):
    """256 instances, 4 steps (per-instance N_i = 1 .. 6 in the first case).  300x80: every instance against the oracle;
    512x256: the fixed subset (every instance still against the streaming path)."""
    kw, stays = INPUTS_C[name]
    kw = dict(kw)
    assert Cm.R_D < 0.04
    n, N = 256, 4
    put = kw.pop("put", False)
    strikes, grids, U0 = _inputs(m1, m2, n, put=put)
    if put:
        kw["put_strikes"] = strikes
    if kw.pop("per", False):
        kw["per"] = _per_instance_draws(n)
        N = 1
    U, d, ds = _resident_and_streaming(solver, m1, m2, N, grids, U0, want_resident=stays, **kw)
    if stays:
        assert "hadi_pass_a_strip<8,EU> (strips of %d rows)" % ((m2 + 8) // 8) in d, d
    else:
        assert "strip" not in d and "hadi_pass_a<8,1" in d and d == ds, (d, ds)
    _oracle_check(m1, m2, grids, U0, U, range(n) if m1 == 300 else SUBSET(n), N=N, **kw)


# ---- D. device memory and the launchers ---------------------------------------------------------------------------
def test_device_memory_path_is_the_resident_kernel_and_equals_the_host_path(solver):
    """As test_gpu_parity.py::test_device_memory_path_equals_host_path, on the batch the resident kernel serves: 256 instances
    of 512x256 in device tensors, bit-identical to the host-array call."""
    import torch
    m1, m2, N, n = 512, 256, 5, 256
    strikes, grids, U0 = _inputs(m1, m2, n)
    U_host, d_host = _run(solver, m1, m2, N, grids, U0, 1)
    assert RESIDENT in d_host, d_host
    dev = torch.device("cuda:0")
    gd = grids.to(dev)
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1), device=dev)
    ws.U.copy_(torch.from_numpy(U0))
    torch.cuda.synchronize()
    solver.set_tuning("resident_sweep", 1)
    try:
        prices = solver.parallel_DO_solve(n, Cm.S_0, Cm.V_0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, gd, ws)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("resident_sweep", -1)
    assert prices.is_cuda and RESIDENT in d and d == d_host, d
    assert np.array_equal(ws.U.cpu().numpy(), U_host)
    g = H.Grid(m1, 8 * strikes[0], Cm.S_0, strikes[0], strikes[0] / 5, m2, 5.0, Cm.V_0, 0.01)
    assert prices.cpu().numpy()[0] == U_host[0, g.find_s_index(Cm.S_0) + g.find_v0_index(Cm.V_0) * (m1 + 1)]


def test_launchers_on_the_resident_kernel(solver):
    """parallel_DO_solve and compute_base_prices with 256 options of 300x80: prices against oracle.base_prices at the bound
    test_gpu_parity.py uses for the same launchers (its PRICE_ATOL)."""
    from test_gpu_parity import PRICE_ATOL
    m1, m2, N, n = 300, 80, 6, 256
    _, grids, U0 = _inputs(m1, m2, n)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, O.EU)
    want, _ = O.base_prices(p, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, threads=16)
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1))
    solver.set_tuning("resident_sweep", 1)
    try:
        ws.U[...] = U0
        prices = solver.parallel_DO_solve(n, Cm.S_0, Cm.V_0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, R_F, *MODEL, grids, ws)
        d1 = solver.describe_last_sweep()
        ws.U[...] = U0
        again = solver.compute_base_prices(Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), N, Cm.THETA,
                                           Cm.T / N, n, grids, ws)
        d2 = solver.describe_last_sweep()
    finally:
        solver.set_tuning("resident_sweep", -1)
    assert RESIDENT in d1 and RESIDENT in d2, (d1, d2)
    print("  launcher prices vs oracle: %.3e, %.3e" % (np.abs(prices - want).max(), np.abs(again - want).max()))
    assert np.abs(prices - want).max() <= PRICE_ATOL and np.abs(again - want).max() <= PRICE_ATOL


# ---- E. long loops ------------------------------------------------------------------------------------------------
def test_thousand_steps_300x80(solver):
    """1000 steps in one launch (the LDS aliasing between the column phase and the next step's ring prologue, a thousand times
    over): resident against streaming, and every instance against the oracle."""
    m1, m2, N, n = 300, 80, 1000, 256
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0)
    _oracle_check(m1, m2, grids, U0, U, range(n), N=N)


def test_thousand_steps_full_size_as_benchmarked(solver):
    """BASELINE config 2 as the benchmark runs it -- 256 instances of 512x256, 1000 steps, canonical parameters (r_f = 0) --
    arranged as 64 groups of (U0, U0 + W_g, W_g, 0): resident against streaming on every instance, the recorded reference
    price, the affine-superposition identity of test_gpu_parity.py::test_full_size_properties_config2 (its 1e-9 bound) in
    every group, the oracle on instances 0 and n - 1 (tens of seconds each), and the step count the timing reports."""
    from test_gpu_parity import PRICE_ATOL
    m1, m2, N, n, K = 512, 256, 1000, 256, 100.0
    _, grids, U0 = _inputs(m1, m2, n, strikes=[K] * n)
    rng = np.random.default_rng(11)
    for g in range(n // 4):
        W = rng.standard_normal(U0.shape[1]) * 3.0
        U0[4 * g + 1] += W
        U0[4 * g + 2] = W
        U0[4 * g + 3] = 0.0
    U, d = _run(solver, m1, m2, N, grids, U0, -1, r_f=Cm.R_F)  # (the benchmarked call: default tuning)
    assert "both passes of every step in one launch: " + RESIDENT in d and "strips of 33 rows" in d, d
    t = solver.timing()
    assert t["point_steps"] == 256 * 513 * 257 * 1000 and t["sweep_ms"] > 0
    Us, ds = _run(solver, m1, m2, N, grids, U0, 0, r_f=Cm.R_F)
    assert RESIDENT not in ds, ds
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("  resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13 and np.isfinite(U).all()
    node = 181 + 78 * (m1 + 1)
    assert abs(U[0, node] - 8.8942192888223310) <= PRICE_ATOL, U[0, node]
    assert 0.0 <= U[0, node] <= Cm.S_0
    worst = 0.0
    for g in range(n // 4):
        lhs, rhs = U[4 * g + 1] - U[4 * g], U[4 * g + 2] - U[4 * g + 3]
        worst = max(worst, np.abs(lhs - rhs).max() / max(1.0, np.abs(rhs).max()))
    print("  affine superposition, worst group: %.3e" % worst)
    assert worst <= 1e-9
    _oracle_check(m1, m2, grids, U0, U, [0, n - 1], N=N, r_f=Cm.R_F, threads=2)


# ---- F. counted waits under load ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,rs", [(400, 263, 33), (400, 131, 17), (400, 64, 9), (512, 100, 13)])
def test_counted_waits_of_the_resident_kernel_under_load_equal_full_drains(solver, strict_solver, m1, m2, rs):
    """The row phase's hand-counted vmcnt waits with every CU busy, at the strip heights that give the different wait
    schedules: 256 instances, 20 steps, bit for bit against the build whose waits drain everything."""
    n, N = 256, 20
    _, grids, U0 = _inputs(m1, m2, n)
    U, d = _run(solver, m1, m2, N, grids, U0, 1)
    Ux, dx = _run(strict_solver, m1, m2, N, grids, U0, 1)
    assert RESIDENT in d and "(strips of %d rows)" % rs in d, d
    assert d == dx
    assert np.array_equal(U, Ux)
    assert np.isfinite(U).all()


# ---- G. captured graphs ---------------------------------------------------------------------------------------------
def test_graph_cache_keeps_the_two_modes_apart(solver):
    """400x31 x256 (one chunk) fits the graph limit, so its time loop -- the resident launch included -- is captured and
    replayed.  The same call twice: the second is a replay, bit-identical.  Then "resident_sweep" 1 -> 0 -> 1 -> 0: the first
    streaming call must CAPTURE (a replay there could only be the resident graph), afterwards each mode replays its own
    cached graph, and the description follows the mode every time.  (N = 7 occurs nowhere else on this shape, and the step
    count is part of the graph key: the counters below are exact.)"""
    m1, m2, N, n = 400, 31, 7, 256
    _, grids, U0 = _inputs(m1, m2, n)
    seen = []
    for mode, want in ((1, {"captures": 1, "replays": 0}), (1, {"captures": 0, "replays": 1}), (0, {"captures": 1, "replays": 0}),
                       (1, {"captures": 0, "replays": 1}), (0, {"captures": 0, "replays": 1})):
        g0 = Cm.graph_counts(solver)
        U, d = _run(solver, m1, m2, N, grids, U0, mode, strip=1)
        dg = Cm.graph_delta(g0, Cm.graph_counts(solver))
        assert (RESIDENT in d) == bool(mode), (mode, d)
        assert {k: dg[k] for k in want} == want, (mode, dg)
        assert dg["drops"] == 0 or not seen, (mode, dg)  # (only the first call may move a buffer -- and with it empty the cache)
        seen.append((mode, U))
    assert all(np.array_equal(U, seen[0][1]) for mode, U in seen if mode == 1)
    assert np.array_equal(seen[2][1], seen[4][1])
    rel = np.abs(seen[0][1] - seen[2][1]).max() / np.abs(seen[2][1]).max()
    print("  resident vs streaming (graph replays), max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13
    _oracle_check(m1, m2, grids, U0, seen[0][1], range(n), N=N)
