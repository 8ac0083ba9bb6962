"""The sampled ladder on the device over its admitted domain: the shapes, sample counts and spot placements of
tests/sample_cases.py (tests/test_emu_sample_domain.py is the same walk under the emulator).  tests/test_gpu_samples.py runs one
case per execution path with ten spots per instance; this file runs
  - every row of event_cases.SHAPES on the streaming kernels with up to 1024 samples per instance (several blocks of
    hadi_sample_locate_kernel / hadi_sample_kernel, 3 n_samp no multiple of 256),
  - every row of LDS_ROWS on the five whole-loop kernels (hadi_small_sch_kernel<2,..> included) and every entry of COUNTS at 50x25,
  - two streams against one bit for bit, DIV / puts / AM_DIV, the Jacobian with 900 columns per instance, the growth of the sample
    buffers under a cached graph and one NaN spot among 1024.
Checks, everywhere: the tight check of sample_cases (interior samples against the node-hit columns of the same call at
32 * 2^-53 sum|w u| |scale|, derived there, not measured); every sample against samples_ref on the oracle's field at the existing
1e-10 sum|w| |scale| max|U_ref| (node hits: sum|w| = 1); the S_0 column against maturity_ladder on the same route bit for bit; the
description's words.  Three instances and N = 4 unless stated; calls run at the canonical r_f = 0."""
import contextlib
import functools

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm
import dividend_schedules as D
import sample_cases as SC
from test_gpu_samples import LOOP, MODEL, STREAM, TH_HV, TH_MCS, Case, _words

pytestmark = pytest.mark.gpu

DEFAULTS = {"small_grid": 1, "small_seq": -1, "small_pairs": -1, "small_sch": -1, "small_waves": 0, "american_p": 1, "streams": 0,
            "strip": -1, "graph": 1}
BLOCK4, BLOCK8 = {"small_seq": 0, "small_waves": 4}, {"small_seq": 0, "small_waves": 8}
SEQ, SEQ2, SCH = {"small_seq": 1, "small_pairs": 0}, {"small_seq": 1, "small_pairs": 1}, {"small_sch": 1}
N_STEPS, SNAPS = 4, [1, 3, 4]
WORST = {"tight": 0.0}


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


@functools.lru_cache(maxsize=None)
def case(m1, m2, n=3, N=N_STEPS, variant="EU", scheme=0, theta=Cm.THETA, put=False):
    """One Case per problem, so that its oracle fields are computed once and shared by the kernels that run it."""
    return Case(m1, m2, n=n, N=N, variant=variant, scheme=scheme, theta=theta, put=put)


def against_oracle(c, out, snaps, spots, scales):
    """Every sample at the existing bound 1e-10 sum|w| |scale| max|U_ref| (vectorised samples_ref.sample_batch: same taps)."""
    import samples_ref as R
    idx, w = SC.stencils(c.grids.Vec_s, spots)
    m1 = c.m1
    for q, N in enumerate(snaps):
        U = c.fields(N)
        for k in range(c.n):
            j0 = R.row_index(c.grids.Vec_v[k], c.v0)
            u = U[k][j0 * (m1 + 1):(j0 + 1) * (m1 + 1)][idx[k]]
            ref = (w[k] * u).sum(axis=-1) * scales[k]
            bound = 1e-10 * np.abs(w[k]).sum(axis=-1) * np.abs(scales[k]) * np.abs(U[k]).max()
            diff = np.abs(out[k, q] - ref)
            assert (diff <= bound).all(), (N, k, np.argwhere(diff > bound)[:4].ravel(), (diff / bound).max())


def domain_check(sv, c, tuning, names, how, snaps=SNAPS, count=None, absent=(), budget=1024):
    spots, scales, kinds = SC.batch_spots(c.grids.Vec_s, Cm.S_0, budget, count)
    n_samp = spots.shape[1]
    with tuned(sv, **tuning):
        out, d = c.samples(sv, snaps, spots=spots, scales=scales)
        assert out.shape == (c.n, len(snaps), n_samp)
        assert _words(snaps, n_samp) + (", " if how == STREAM else " ") + how in d and all(x in d for x in names), d
        assert not any(x in d for x in absent), d
        lad, d1 = c.ladder(sv, snaps)
        assert "maturity ladder" in d1 and all(x in d1 for x in names), d1
    assert np.array_equal(out[:, :, 0], lad), out[:, :, 0] - lad
    worst, checked = SC.tight_check(out, c.grids.Vec_s, spots, scales, d[:60])
    assert checked == int(((kinds == SC.INTERIOR) | (kinds == SC.TOL_INTERIOR)).sum())
    against_oracle(c, out, snaps, spots, scales)
    WORST["tight"] = max(WORST["tight"], worst)
    print("TIGHT %dx%d n_samp %d %s | %.3f (file so far %.3f)" % (c.m1, c.m2, n_samp, d[:50], worst, WORST["tight"]))
    return out


# ---- streaming shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SC.SHAPES, ids=["%s-%dx%d" % (s.name, s.m1, s.m2) for s in SC.SHAPES])
def test_streaming_shapes(solver, s):
    c = case(s.m1, s.m2)
    # (budget 1023: the lists of the rows above 252 intervals fill it, and 3 * 1024 would be whole blocks)
    out = domain_check(solver, c, {"small_grid": 0}, ["row pass"], STREAM, absent=["hadi_small_"], budget=1023)
    n_samp = out.shape[2]
    assert n_samp > 256 or s.m1 < 64, n_samp  # several blocks of the two sample kernels
    assert (3 * n_samp) % 256 != 0


# ---- whole-loop kernels ---------------------------------------------------------------------------------------------------------
LDS_PATHS = [("block4", BLOCK4, "hadi_small_kernel<%d,4,EU>", 0), ("block8", BLOCK8, "hadi_small_kernel<%d,8,EU>", 0),
             ("seq", SEQ, "hadi_small_seq_kernel<%d>", 0), ("pairs", SEQ2, "hadi_small_seq2_kernel<%d>", 0),
             ("sch-MCS", SCH, "hadi_small_sch_kernel<%d,MCS>", H.SCHEME_MCS)]
SCHEME_THETA = {0: Cm.THETA, H.SCHEME_CRAIG_SNEYD: 0.5, H.SCHEME_MCS: TH_MCS, H.SCHEME_HV: TH_HV}


@pytest.mark.parametrize("pname,tuning,kernel,scheme", LDS_PATHS, ids=[p[0] for p in LDS_PATHS])
@pytest.mark.parametrize("m1,m2", SC.LDS_ROWS, ids=["%dx%d" % r for r in SC.LDS_ROWS])
def test_lds_shapes(solver, m1, m2, pname, tuning, kernel, scheme):
    B = SC.pick_shape(m1)[0]
    absent = []
    if pname == "pairs" and m2 + 1 > 32:  # the pairs kernel holds at most 32 v-rows: small_pairs = 1 runs the one-instance kernel
        kernel, absent = "hadi_small_seq_kernel<%d>", ["seq2"]
    domain_check(solver, case(m1, m2, scheme=scheme, theta=SCHEME_THETA[scheme]), tuning, [kernel % B], LOOP, absent=absent)


@pytest.mark.parametrize("scheme,name", [(H.SCHEME_CRAIG_SNEYD, "CS"), (H.SCHEME_HV, "HV")], ids=["CS", "HV"])
def test_scheme_kernel_with_two_nodes_per_lane(solver, scheme, name):
    domain_check(solver, case(128, 20, scheme=scheme, theta=SCHEME_THETA[scheme]), SCH, ["hadi_small_sch_kernel<2,%s>" % name], LOOP)


@pytest.mark.parametrize("pname,tuning,kernel,scheme", LDS_PATHS, ids=[p[0] for p in LDS_PATHS])
def test_every_sample_count_at_50x25(solver, pname, tuning, kernel, scheme):
    c = case(50, 25, scheme=scheme, theta=SCHEME_THETA[scheme])
    for count in SC.COUNTS:
        domain_check(solver, c, tuning, [kernel % 1], LOOP, count=count)


# ---- two streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samp", [257, 1024])
@pytest.mark.parametrize("m1,m2", [(50, 25), (300, 20)], ids=["50x25", "300x20"])
def test_two_streams_against_one(solver, m1, m2, n_samp):
    c = case(m1, m2, n=5)
    spots, scales, _ = SC.batch_spots(c.grids.Vec_s, Cm.S_0, n_samp, n_samp)
    with tuned(solver, small_grid=0, streams=2):
        two, d2 = c.samples(solver, SNAPS, spots=spots, scales=scales)
    with tuned(solver, small_grid=0, streams=1):
        one, d1 = c.samples(solver, SNAPS, spots=spots, scales=scales)
    assert "side by side on two streams" in d2 and "side by side" not in d1 and STREAM in d1 and STREAM in d2, (d1, d2)
    assert np.array_equal(one, two)
    worst, _ = SC.tight_check(two, c.grids.Vec_s, spots, scales, "two streams")
    against_oracle(c, two, SNAPS, spots, scales)
    WORST["tight"] = max(WORST["tight"], worst)
    print("TIGHT two streams %dx%d n_samp %d | %.3f" % (m1, m2, n_samp, worst))


# ---- variants -------------------------------------------------------------------------------------------------------------------
def test_dividends_on_the_streaming_path_with_snapshots_on_paying_steps(solver):
    N, snaps = 10, [2, 4, 10]
    assert sorted(D.paying_steps(N, Cm.T / N, Cm.DIVS[0])) == [2, 4, 8]
    domain_check(solver, case(100, 20, N=N, variant="DIV"), {"small_grid": 0}, ["row pass"], STREAM, snaps=snaps)


def test_puts_on_the_streaming_path(solver):
    domain_check(solver, case(100, 20, put=True), {"small_grid": 0}, ["row pass"], STREAM)


@pytest.mark.parametrize("tuning,names,how", [(BLOCK4, ["hadi_small_kernel<1,4,AM>"], LOOP), ({"small_grid": 0, "american_p": 1}, ["row pass"], STREAM)],
                         ids=["block", "streaming"])
def test_american_with_dividends(solver, tuning, names, how):
    N, snaps = 10, [2, 4, 10]
    out = domain_check(solver, case(50, 25, N=N, variant="AM_DIV", put=True), tuning, names, how, snaps=snaps)
    assert np.isfinite(out).all()


# ---- Jacobian: 900 columns per instance ---------------------------------------------------------------------------------------
def _jac_spots():
    """The golden Jacobian's shape, N and eps on well-conditioned strikes (its own strikes put K a hair beside a node: sum|w| = 54
    in the interval next to it, beyond what domain_spots admits)."""
    j = Cm.GOLDEN["jacobian"]
    strikes = Cm.well_conditioned_strikes(j["m1"], len(j["strikes"]))
    grids = H.GridViewsBatch.for_strikes(j["m1"], j["m2"], Cm.S_0, Cm.V_0, strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(strikes)
    spots, scales, _ = SC.batch_spots(grids.Vec_s, Cm.S_0, 300, 300)
    return j, strikes, grids, U0, spots, scales


def test_jacobian_on_a_whole_loop_route_bit_for_bit(solver):
    """Against six compute_base_prices_samples calls with the parameters moved by eps in turn (the same v-grid rebuild)."""
    j, strikes, grids, U0, spots, scales = _jac_spots()
    m1, m2, N, n, eps = j["m1"], j["m2"], j["N"], len(strikes), j["eps"]
    total, snaps = (m1 + 1) * (m2 + 1), [5, 12, 20]
    rho, sigma, kappa, eta = MODEL
    with tuned(solver, small_seq=1, small_pairs=0):
        J, base = solver.compute_jacobian_samples(spots, Cm.V_0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, total, N, Cm.THETA,
                                                  Cm.T / N, n, grids, U0, snaps, scales=scales, eps=eps)
        d = solver.describe_last_sweep()
        assert J.shape == (n, 3, 300, 5) and base.shape == (n, 3, 300) and 3 * 300 > 3 * 256
        assert _words(snaps, 300) in d and "hadi_small_seq_kernel<" in d, d
        ws = H.DOWorkspace(n, total)

        def one(v0, rho, sigma, kappa, eta):
            ws.U[...] = U0
            out = solver.compute_base_prices_samples(spots, v0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, total, N, Cm.THETA,
                                                     Cm.T / N, n, grids, ws, snaps, scales=scales)
            assert "hadi_small_seq_kernel<" in solver.describe_last_sweep()
            return out

        b = one(Cm.V_0, rho, sigma, kappa, eta)
        assert np.array_equal(base, b)
        moved = [one(Cm.V_0, rho, sigma, kappa + eps, eta), one(Cm.V_0, rho, sigma, kappa, eta + eps),
                 one(Cm.V_0, rho, sigma + eps, kappa, eta), one(Cm.V_0, rho + eps, sigma, kappa, eta),
                 one(Cm.V_0 + eps, rho, sigma, kappa, eta)]
        for c, pert in enumerate(moved):
            assert np.array_equal(J[..., c], (pert - b) / eps), c
    worst, _ = SC.tight_check(base, grids.Vec_s, spots, scales, "jacobian base")
    print("TIGHT jacobian base | %.3f" % worst)
    WORST["tight"] = max(WORST["tight"], worst)


def test_jacobian_on_the_streaming_route_vs_oracle(solver):
    """The tolerances of test_gpu_samples.test_jacobian_samples_on_the_streaming_path_vs_oracle: prices 1e-9, J 2e-4 (2e-5 on the
    first three instances), against the oracle's own forward differences of sampled fields."""
    from oracle import oracle as O
    import samples_ref as R
    j, strikes, grids, U0, spots, _ = _jac_spots()  # (scale 1: the existing tolerances are stated for unscaled prices)
    m1, m2, N, n, eps = j["m1"], j["m2"], j["N"], len(strikes), j["eps"]
    snaps = [5, 12, 20]
    rho, sigma, kappa, eta = MODEL
    with tuned(solver, small_grid=0):
        J, base = solver.compute_jacobian_samples(spots, Cm.V_0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, (m1 + 1) * (m2 + 1), N,
                                                  Cm.THETA, Cm.T / N, n, grids, U0, snaps, eps=eps)
        assert "hadi_sample_kernel" in solver.describe_last_sweep()
    idx, w = SC.stencils(grids.Vec_s, spots)

    def ref(Nq, v0, rho, sigma, kappa, eta):
        vv, dv = O.rebuild_variance(m2, v0)
        p = O.make_params(m1, m2, Nq, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, O.EU)
        U = O.solve_batch(p, grids.Vec_s, np.tile(vv, (n, 1)), grids.Delta_s, np.tile(dv, (n, 1)), U0)[0]
        j0 = R.row_index(vv, v0)
        u = np.stack([U[k][j0 * (m1 + 1):(j0 + 1) * (m1 + 1)][idx[k]] for k in range(n)])
        return ((((w[..., 0] * u[..., 0]) + w[..., 1] * u[..., 1]) + w[..., 2] * u[..., 2]) + w[..., 3] * u[..., 3])

    for q, Nq in enumerate(snaps):
        b = ref(Nq, Cm.V_0, rho, sigma, kappa, eta)
        moved = [ref(Nq, Cm.V_0, rho, sigma, kappa + eps, eta), ref(Nq, Cm.V_0, rho, sigma, kappa, eta + eps),
                 ref(Nq, Cm.V_0, rho, sigma + eps, kappa, eta), ref(Nq, Cm.V_0, rho + eps, sigma, kappa, eta),
                 ref(Nq, Cm.V_0 + eps, rho, sigma, kappa, eta)]
        Jo = np.stack([(m - b) / eps for m in moved], axis=-1)
        assert np.abs(base[:, q] - b).max() <= 1e-9
        assert np.abs(J[:, q] - Jo).max() <= 2e-4 and np.abs(J[:3, q] - Jo[:3]).max() <= 2e-5, Nq
    worst, _ = SC.tight_check(base, grids.Vec_s, spots, np.ones_like(spots), "jacobian base, streaming")
    print("TIGHT jacobian base, streaming | %.3f" % worst)
    WORST["tight"] = max(WORST["tight"], worst)


# ---- growth of the sample buffers under a cached graph, on a handle of its own --------------------------------------------------
def test_sample_buffers_grow_under_a_cached_graph():
    """A (n_samp = 10) captures its loop; B (n_samp = 1024, the same batch) must grow samp_in / samp_tap / samp_out, which frees
    the buffers A's graph holds: the cache is dropped then and only then, and the second A is a fresh capture with A's bits."""
    c = case(100, 20, n=5)
    sa, ca, _ = SC.batch_spots(c.grids.Vec_s, Cm.S_0, 1024, 10)
    sb, cb, _ = SC.batch_spots(c.grids.Vec_s, Cm.S_0, 1024, 1024)
    with H.HestonADI(0) as h:
        h.set_tuning("small_grid", 0)
        h.set_tuning("graph", 1)
        counts, got = [Cm.graph_counts(h)], []
        for spots, scales in ((sa, ca), (sb, cb), (sa, ca), (sb, cb), (sa, ca)):
            out, d = c.samples(h, SNAPS, spots=spots, scales=scales)
            assert STREAM in d, d
            got.append(out)
            counts.append(Cm.graph_counts(h))
    a1, b1, a2, b2, a3 = (Cm.graph_delta(counts[k], counts[k + 1]) for k in range(5))
    assert (a1["captures"], a1["replays"]) == (1, 0), a1
    assert b1["drops"] >= 1 and (b1["captures"], b1["replays"]) == (1, 0), b1        # the sample buffers grew: the cache was emptied
    assert (a2["captures"], a2["replays"], a2["drops"]) == (1, 0, 0), a2              # a fresh capture, not a replay over freed buffers
    assert (b2["captures"], b2["replays"], b2["drops"]) == (0, 1, 0), b2              # nothing grows any more: nothing is dropped
    assert (a3["captures"], a3["replays"], a3["drops"]) == (0, 1, 0), a3
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[4]) and np.array_equal(got[1], got[3])
    assert np.array_equal(got[0], got[1][:, :, :10])  # (A's list is the head of B's)
    worst, _ = SC.tight_check(got[1], c.grids.Vec_s, sb, cb, "growth B")
    against_oracle(c, got[1], SNAPS, sb, cb)
    print("TIGHT growth B | %.3f" % worst)
    WORST["tight"] = max(WORST["tight"], worst)


# ---- off the grid -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{"small_grid": 0}, SEQ2], ids=["streaming", "pairs"])
def test_one_nan_spot_among_1024(solver, tuning):
    c = case(50, 25)
    spots, scales, _ = SC.batch_spots(c.grids.Vec_s, Cm.S_0, 1024, 1024)
    with tuned(solver, **tuning):
        good, _ = c.samples(solver, SNAPS, spots=spots, scales=scales)
        off = spots.copy()
        off[2, 700] = np.nan
        # the raw entry point: the status AND the outputs (the wrapper raises)
        import ctypes as C
        from pde_based_heston_solver_gpu_accelerated_amd import _native as nat
        p = solver._problem(H.EU, *c.head()[:11], c.grids, U=c.U0.copy())
        steps = np.array(SNAPS, dtype=np.int32)
        out = np.zeros((3, len(SNAPS), 1024))
        dp = lambda a: a.ctypes.data_as(nat._dp)
        sc = np.ascontiguousarray(scales)
        st = nat.Samples(1024, dp(off), dp(sc), 3)
        rc = solver._lib.hadi_sample_ladder(solver._h, C.byref(p), c.v0, C.byref(st), len(SNAPS), steps.ctypes.data_as(C.POINTER(C.c_int)),
                                            C.c_void_p(out.ctypes.data))
    assert rc == 4  # HADI_ERR_NOT_ON_GRID
    bad = np.zeros(out.shape, dtype=bool)
    bad[2, :, 700] = True
    assert np.isnan(out[bad]).all() and np.array_equal(out[~bad], good[~bad])
