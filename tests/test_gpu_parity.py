"""GPU parity tests: libhadi (hand-written gfx950 kernels, through the C ABI) against the CPU oracle on
the same seeded inputs, against the reference outputs recorded in tests/golden, and -- at BASELINE.json's
full sizes, where the oracle is too slow -- through size-independent properties.

Tolerances (fp64 everywhere; north_star asks price error < 1e-6):
  full field  max|U - U_oracle| <= 1e-10 * max|U_oracle|   (observed ~1e-14)
  prices      |p - p_ref| <= 1e-9                           (observed ~1e-13)
  Jacobian    forward differences with eps = 1e-6 amplify price round-off by 1e6.  On the reference's
              25x20 test grid the K = 94 instance has a 0.038-wide s-interval next to a 5.4-wide one
              (S_0 lands beside a node), which conditions its operators badly: oracle and libhadi each
              carry ~1e-11 of round-off there, so J agrees to ~4e-5 on that row (1e-7 on the others):
              atol 2e-4; the row the reference printed (K = 90) is checked to 2e-5
The only differences from the oracle are operation order (partition / cyclic-reduction line solves,
FMA contraction, factored coefficients); there is no approximation in the scheme.
"""
import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm

pytestmark = pytest.mark.gpu

FIELD_RTOL = 1e-10
PRICE_ATOL = 1e-9


@pytest.fixture
def forced_strips(solver):
    """The strip row pass forced through hadi_set_tuning for the duration of one test (the plan picks it by itself for
    large batches only)."""
    solver.set_tuning("strip", 1)
    yield solver
    solver.set_tuning("strip", -1)


def _batch(m1, m2, strikes):
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    return grids, grids.call_payoff(strikes)


def _hadi_solve(solver, m1, m2, N, strikes, variant, r_f=Cm.R_F, want_lambda=False, T=Cm.T, per_instance=None,
                model=None):
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    lam = np.zeros_like(U) if want_lambda else None
    div = H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None
    rho, sigma, kappa, eta = model or (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
    solver.DO_timestepping(m1, m2, N, T / N, Cm.THETA, Cm.R_D, r_f, rho, sigma, kappa, eta, grids, U,
                           variant=variant, U_0=U0, lambda_bar=lam, dividends=div, per_instance=per_instance)
    return grids, U0, U, lam


def _assert_field(U, Uo, rtol=FIELD_RTOL):
    scale = np.abs(Uo).max()
    err = np.abs(U - Uo).max()
    assert err <= rtol * scale, "field error %.3e (scale %.3e)" % (err, scale)


SHAPES = [
    # m1, m2, N, n_inst           what it exercises
    (50, 25, 20, 5),            # reference calibration grid: 1 node/lane, single chunk
    (100, 50, 200, 1),          # BASELINE config 1
    (40, 12, 7, 3),             # tiny, idle lanes
    (33, 20, 5, 2),             # odd sizes
    (64, 33, 6, 2),             # m1 exactly one wave
    (65, 40, 6, 2),             # 2 nodes/lane, mostly padding
    (128, 64, 10, 3),           # 2 nodes/lane full
    (200, 100, 40, 2),          # 4 nodes/lane, 2 chunks
    (130, 70, 6, 2),            # 4 nodes/lane, ragged
    (256, 128, 12, 3),          # BASELINE config 3 grid
    (512, 256, 8, 2),           # BASELINE config 2 grid (few steps so the oracle finishes in seconds)
    (300, 140, 5, 1),           # 8 nodes/lane with padding, 5 chunks
    (1024, 512, 4, 1),          # BASELINE config 5 grid: two wavefronts per row (split solve), 16 chunks
    (700, 300, 4, 2),           # two wavefronts per row, ragged
]


@pytest.mark.parametrize("m1,m2,N,n", SHAPES)
def test_european_full_field_vs_oracle(solver, m1, m2, N, n):
    strikes = Cm.strikes_for(n)
    grids, U0, U, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU)
    p = Cm.oracle_params(m1, m2, N, "EU")
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


@pytest.mark.parametrize("variant,name", [(H.AM, "AM"), (H.DIV, "DIV"), (H.AM_DIV, "AM_DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 20, 4), (256, 128, 25, 2), (130, 70, 20, 2)])
def test_american_dividend_variants_vs_oracle(solver, variant, name, m1, m2, N, n):
    strikes = Cm.strikes_for(n)
    grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, want_lambda=variant in (H.AM, H.AM_DIV))
    p = Cm.oracle_params(m1, m2, N, name)
    Uo, lamo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    if lamo is not None:
        # lambda_bar = max(0, lambda + (U_0 - U_bar)/dt): a field error e shows up as e/dt
        assert np.abs(lam - lamo).max() <= 1e-8 * max(1.0, np.abs(lamo).max())


@pytest.mark.parametrize("american_p", [1, 0], ids=["P", "explicit"])
@pytest.mark.parametrize("variant,name", [(H.AM, "AM"), (H.AM_DIV, "AM_DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(100, 50, 30, 2), (256, 128, 25, 3), (512, 256, 12, 2), (700, 300, 6, 1), (1024, 512, 4, 1)])
def test_american_p_representation_and_explicit_pair(solver, american_p, variant, name, m1, m2, N, n):
    """American sweeps store P = U_bar - dt lambda_bar_old in place of U and rebuild U = max(P, U0), lambda_bar =
    max(0, (U0 - P)/dt) on the fly (no lambda_bar array) whenever the payoff depends on s only; the first step and
    dividend steps run on the explicit (U, lambda_bar) pair.  Both ways must give the oracle's U and lambda_bar; r_f != 0
    and N = 25..30 put several dividend steps and conversions into the loop."""
    strikes = Cm.strikes_for(n)
    solver.set_tuning("american_p", american_p)
    try:
        grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, r_f=0.01, want_lambda=True)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("american_p", 1)
    assert ("AM-P" in d) == bool(american_p)
    p = Cm.oracle_params(m1, m2, N, name, r_f=0.01)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("m1,m2,N,n", [(256, 128, 25, 4), (50, 25, 20, 3)])
def test_put_shaped_payoff_american_with_dividends(solver, m1, m2, N, n):
    """BASELINE config 3 speaks of American puts with dividends; the reference has no put path (its boundary vectors are
    call-type), but the stepper is payoff-agnostic: with U_0 = max(K - s, 0) libhadi must reproduce the oracle -- the
    reference's algorithm on the same input -- exactly as for calls, including the projection against this payoff."""
    strikes = Cm.strikes_for(n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.put_payoff(strikes)
    U, lam = U0.copy(), np.zeros_like(U0)
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                           variant=H.AM_DIV, U_0=U0, lambda_bar=lam, dividends=H.Dividends(*Cm.DIVS))
    p = Cm.oracle_params(m1, m2, N, "AM_DIV")
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())
    assert lo.max() > 0  # the early-exercise constraint is active for this payoff


@pytest.mark.parametrize("m1,m2,N,n", [(256, 128, 10, 3), (512, 256, 5, 2), (1024, 512, 3, 1), (50, 25, 10, 2)])
def test_american_with_a_payoff_that_depends_on_v(solver, m1, m2, N, n):
    """The column pass loads a payoff that depends on s only (every driver of the reference) once per column; a general
    U_0 must take the per-node path and still match the oracle.  The same batch mixes both kinds of instance."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U0 = U0.reshape(n, m2 + 1, m1 + 1).copy()
    U0[0] += 0.5 * grids.Vec_v[0][:, None] * (grids.Vec_s[0][None, :] > strikes[0])  # instance 0: v-dependent payoff
    U0 = np.ascontiguousarray(U0.reshape(n, -1))
    U, lam = U0.copy(), np.zeros_like(U0)
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                           variant=H.AM, U_0=U0, lambda_bar=lam)
    p = Cm.oracle_params(m1, m2, N, "AM")
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("variant,name", [(H.EU, "EU"), (H.AM, "AM"), (H.DIV, "DIV"), (H.AM_DIV, "AM_DIV")])
def test_small_grid_kernel_and_streaming_kernels_agree(solver, variant, name):
    """Grids that fit in LDS run through the one-launch LDS-resident kernel by default; the two-pass
    streaming kernels must give the same field (both within 1e-10 of the oracle, 1e-11 of each other),
    with and without hipGraph replay of the time loop."""
    m1, m2, N, strikes = 50, 25, 20, Cm.strikes_for(6)
    p = Cm.oracle_params(m1, m2, N, name)
    fields = []
    for small, graph, seq in ((1, 1, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0)):
        solver.set_tuning("small_grid", small)
        solver.set_tuning("graph", graph)
        solver.set_tuning("small_seq", seq)  # (European / dividends: sequential one-wavefront kernel or the block kernel)
        try:
            g0 = Cm.graph_counts(solver)
            grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, want_lambda=variant in (H.AM, H.AM_DIV))
            dg = Cm.graph_delta(g0, Cm.graph_counts(solver))
        finally:
            solver.set_tuning("small_grid", 1)
            solver.set_tuning("graph", 1)
            solver.set_tuning("small_seq", -1)
        # only the streaming run with graphs on goes through the cache (captured or replayed); the others launch directly
        assert dg["captures"] + dg["replays"] == (1 if (small, graph) == (0, 1) else 0), ((small, graph, seq), dg)
        fields.append((U, lam))
    Uo, lamo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    for U, lam in fields:
        _assert_field(U, Uo)
        if lamo is not None:
            assert np.abs(lam - lamo).max() <= 1e-8 * max(1.0, np.abs(lamo).max())
    assert np.abs(fields[0][0] - fields[1][0]).max() <= 1e-11 * np.abs(Uo).max()
    assert np.abs(fields[0][0] - fields[3][0]).max() <= 1e-11 * np.abs(Uo).max()
    assert np.array_equal(fields[1][0], fields[2][0])  # graph replay == direct launches, bit for bit


@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 20, 4), (128, 64, 8, 2), (512, 256, 6, 2), (700, 300, 3, 1)])
def test_craig_sneyd_vs_oracle(solver, m1, m2, N, n):
    """Craig-Sneyd on the device (N3: the reference has it host-side only, solver.hpp:781-907) against the
    oracle's restatement, full field, incl. the streaming kernels at 1 and 2 wavefronts per row."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    solver.CS_scheme(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.007, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=0.007)
    p.scheme = 1
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


def test_craig_sneyd_reference_price_and_restrictions(solver):
    c = Cm.GOLDEN["craig_sneyd"]
    m1, m2, N, K = c["m1"], c["m2"], c["N"], float(c["K"])
    grids, U0 = _batch(m1, m2, [K])
    U = U0.copy()
    solver.CS_scheme(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
    g = H.Grid(m1, 8 * K, Cm.S_0, K, K / 5, m2, 5.0, Cm.V_0, 0.01)
    price = U[0, g.find_s_index(Cm.S_0) + g.find_v0_index(Cm.V_0) * (m1 + 1)]
    assert abs(price - c["price"]) <= PRICE_ATOL
    with pytest.raises(H.HadiError) as e:  # European only, as in the reference
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids,
                               U0.copy(), variant=H.AM, U_0=U0, scheme=1)
    assert e.value.status == 2


def test_foreign_rate_boundary_terms(solver):
    """r_f != 0 switches on the time-dependent boundary factors exp(r_f dt n) (device_solver.hpp:238-247)
    that every reference test leaves at 1."""
    m1, m2, N, strikes = 70, 30, 12, [90.0, 105.0]
    grids, U0, U, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU, r_f=0.013)
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=0.013)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


def test_upwind_rows_are_exercised(solver):
    """sigma large enough that the v > 1 upwind block (hes_a2_shuffled_kernels.hpp:129-144) matters,
    compared on the full field (the price node alone is blind to those rows)."""
    m1, m2, N, strikes = 60, 40, 10, [100.0]
    model = (-0.5, 0.9, 3.0, 0.3)
    grids, U0, U, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU, model=model)
    assert (grids.Vec_v > 1.0).sum() >= 5
    p = Cm.oracle_params(m1, m2, N, "EU", rho=model[0], sigma=model[1], kappa=model[2], eta=model[3])
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


GOLD = Cm.GOLDEN["prices"]


@pytest.mark.parametrize("case", GOLD, ids=lambda c: "%s_%dx%dx%d_K%s" % (c["variant"], c["m1"], c["m2"], c["N"], c["K"]))
def test_reference_recorded_prices(solver, case):
    """Every reference output recorded for this path, incl. BASELINE config 2
    (512x256, 1000 steps) and the config-3 sized American+dividend call, through the mirrored
    launchers compute_base_prices*."""
    m1, m2, N, K = case["m1"], case["m2"], case["N"], float(case["K"])
    grids, U0 = _batch(m1, m2, [K])
    ws = H.DOWorkspace(1, (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    args = (Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, m1, m2, (m1 + 1) * (m2 + 1), N,
            Cm.THETA, Cm.T / N, 1, grids)
    div = H.Dividends(*Cm.DIVS)
    v = case["variant"]
    if v == "EU":
        price = solver.compute_base_prices(*args, ws)
    elif v == "AM":
        price = solver.compute_base_prices_american(*args, U0, ws)
    elif v == "DIV":
        price = solver.compute_base_prices_dividends(*args, ws, div)
    else:
        price = solver.compute_base_prices_american_dividends(*args, U0, ws, div)
    assert abs(price[0] - case["price"]) <= PRICE_ATOL, (price[0], case["price"])


def test_parallel_DO_solve_matches_compute_base_prices_and_oracle(solver):
    m1, m2, N, n = 50, 25, 20, 20
    strikes = [85.0 + i for i in range(n)]  # device_solver.cpp:624-627
    grids, U0 = _batch(m1, m2, strikes)
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    prices = solver.parallel_DO_solve(n, Cm.S_0, Cm.V_0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F,
                                      Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, ws)
    p = Cm.oracle_params(m1, m2, N, "EU")
    want, _ = O.base_prices(p, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    assert np.abs(prices - want).max() <= PRICE_ATOL
    # the three strikes the reference's own test prints (device_solver.cpp:780)
    for k, ref in enumerate((19.36766348353193, 18.57361239232885, 17.7901173119001)):
        assert abs(prices[k] - ref) < 1e-9
    ws.U[...] = U0
    again = solver.compute_base_prices(Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA,
                                       m1, m2, (m1 + 1) * (m2 + 1), N, Cm.THETA, Cm.T / N, n, grids, ws)
    assert np.abs(again - prices).max() <= 1e-12


@pytest.mark.parametrize("variant", ["EU", "AM", "DIV", "AM_DIV"])
def test_jacobian_vs_oracle(solver, variant):
    j = Cm.GOLDEN["jacobian"]
    m1, m2, N = j["m1"], j["m2"], j["N"]
    strikes = [float(k) for k in j["strikes"]]
    grids, U0 = _batch(m1, m2, strikes)
    args = (Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, m1, m2, (m1 + 1) * (m2 + 1), N,
            Cm.THETA, Cm.T / N, len(strikes), grids, U0)
    div = H.Dividends(*Cm.DIVS)
    if variant == "EU":
        J, base = solver.compute_jacobian(*args, eps=j["eps"])
    elif variant == "AM":
        J, base = solver.compute_jacobian_american(*args, eps=j["eps"])
    elif variant == "DIV":
        J, base = solver.compute_jacobian_dividends(*args, div, eps=j["eps"])
    else:
        J, base = solver.compute_jacobian_american_dividends(*args, div, eps=j["eps"])
    p = Cm.oracle_params(m1, m2, N, variant)
    Jo, baseo = O.jacobian(p, Cm.S_0, Cm.V_0, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, eps=j["eps"])
    assert np.abs(base - baseo).max() <= PRICE_ATOL
    assert np.abs(J - Jo).max() <= 2e-4, np.abs(J - Jo).max()
    assert np.abs(J[:3] - Jo[:3]).max() <= 2e-5
    if variant == "EU":  # the row the reference printed
        assert abs(base[0] - j["base_price_0"]) <= PRICE_ATOL
        assert np.abs(J[0] - np.array(j["J_row_0"])).max() <= 2e-5


def test_per_instance_parameters_and_maturities(solver):
    """Per-instance model parameters (the flattened Jacobian needs them) and per-instance (N, delta_t)
    (multi-maturity calibration, heston_calibration.cpp:2165-2171): each instance must equal an
    individual oracle solve."""
    m1, m2 = 60, 30
    strikes = [90.0, 100.0, 110.0, 95.0]
    Ts = [0.5, 1.0, 2.0, 0.25]
    Ns = [10, 20, 40, 5]
    rhos, sigmas = [-0.9, -0.5, 0.0, 0.3], [0.3, 0.5, 0.2, 0.4]
    kappas, etas = [1.5, 2.0, 0.5, 3.0], [0.04, 0.09, 0.02, 0.06]
    per = {"rho_i": rhos, "sigma_i": sigmas, "kappa_i": kappas, "eta_i": etas, "N_i": Ns,
           "delta_t_i": [t / n for t, n in zip(Ts, Ns)]}
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    solver.DO_timestepping(m1, m2, 1, 1.0, Cm.THETA, Cm.R_D, Cm.R_F, 0.0, 0.1, 1.0, 0.04, grids, U, per_instance=per)
    for k in range(len(strikes)):
        p = O.make_params(m1, m2, Ns[k], Ts[k] / Ns[k], Cm.THETA, Cm.R_D, Cm.R_F, rhos[k], sigmas[k], kappas[k], etas[k])
        Uo, _, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k])
        _assert_field(U[k], Uo)


@pytest.mark.parametrize("variant,kind", [(H.EU, "EU"), (H.AM, "AM-P")])
@pytest.mark.parametrize("m1,m2,tuning,want", [
    (200, 60, {"strip": 1, "pair_strips": 0}, "hadi_pass_a_strip<4,%s>"), (300, 80, {"strip": 1}, "hadi_pass_a_strip<8,%s>"),
    (600, 40, {"strip": 1}, "hadi_pass_a_strip<8,%s,double,2>"), (256, 128, {"strip": 1, "pair_strips": 1}, "hadi_pass_a_pairs<%s>")])
def test_per_instance_maturities_on_strips(solver, variant, kind, m1, m2, tuning, want):
    """Douglas multi-maturity batches with per-instance model parameters on the strip kernels (4 and 8 nodes per lane, paired
    strips, two strips per wavefront), European and American in the P representation: the blocks of the instances that have
    taken their last step leave the row pass early (after draining their row fetches) beside blocks that go on."""
    strikes = [90.0, 100.0, 110.0, 95.0]
    Ts, Ns = [0.5, 1.0, 0.8, 0.25], [5, 8, 3, 1]
    rhos, sigmas, kappas, etas = [-0.9, -0.5, 0.0, 0.3], [0.3, 0.5, 0.2, 0.4], [1.5, 2.0, 0.5, 3.0], [0.04, 0.09, 0.02, 0.06]
    per = {"rho_i": rhos, "sigma_i": sigmas, "kappa_i": kappas, "eta_i": etas, "N_i": Ns,
           "delta_t_i": [t / n for t, n in zip(Ts, Ns)]}
    grids, U0 = _batch(m1, m2, strikes)
    U, lam = U0.copy(), np.zeros_like(U0)
    american = variant == H.AM
    tuning = dict(tuning, team_launch=0, small_grid=0)
    for k, v in tuning.items():
        solver.set_tuning(k, v)
    try:
        solver.DO_timestepping(m1, m2, 1, 1.0, Cm.THETA, Cm.R_D, 0.01, 0.0, 0.1, 1.0, 0.04, grids, U, variant=variant,
                               U_0=U0 if american else None, lambda_bar=lam if american else None, per_instance=per)
        d = solver.describe_last_sweep()
    finally:
        for k in tuning:
            solver.set_tuning(k, -1)
    assert want % kind in d, d
    for k in range(len(strikes)):
        p = O.make_params(m1, m2, Ns[k], Ts[k] / Ns[k], Cm.THETA, Cm.R_D, 0.01, rhos[k], sigmas[k], kappas[k], etas[k], variant)
        Uo, lo, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k], U0[k])
        _assert_field(U[k], Uo)
        if american:
            assert np.abs(lam[k] - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("variant", [H.DIV, H.AM_DIV], ids=["DIV", "AM_DIV"])
@pytest.mark.parametrize("m1,m2,path", [(50, 25, "small"), (50, 25, "graph"), (50, 25, "stream"), (150, 60, "graph"), (150, 60, "auto")])
def test_dividends_with_per_instance_maturities(solver, variant, m1, m2, path):
    """Multi-maturity batches with a shared dividend schedule (compute_*_multi_maturity_american_dividends,
    heston_calibration.cpp:2936-3243): every instance pays the dividends on ITS OWN step grid (n*dt_k evaluated in
    floating point), short maturities skip the late dates.  Each execution path against individual oracle solves."""
    strikes = [90.0, 100.0, 110.0, 95.0, 105.0]
    Ts = [0.5, 1.0, 1.5, 0.25, 0.7]
    Ns = [10, 20, 30, 20, 23]
    per = {"N_i": Ns, "delta_t_i": [t / n for t, n in zip(Ts, Ns)]}
    grids, U0 = _batch(m1, m2, strikes)
    U, lam = U0.copy(), np.zeros_like(U0)
    div = H.Dividends(*Cm.DIVS)
    solver.set_tuning("small_grid", 1 if path == "small" else 0)
    solver.set_tuning("graph", 0 if path == "stream" else 1)
    # ("graph": the captured time loop, so not the instance-resident kernel that the default picks for a few European
    # instances of 150x60; "auto": whatever the default picks)
    solver.set_tuning("team_launch", 0 if path == "graph" else -1)
    try:
        for call in range(2 if path == "graph" else 1):  # second call replays the cached graph
            U[...] = U0
            g0 = Cm.graph_counts(solver)
            solver.DO_timestepping(m1, m2, 1, 1.0, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                                   variant=variant, U_0=U0, lambda_bar=lam if variant == H.AM_DIV else None,
                                   dividends=div, per_instance=per)
            dg = Cm.graph_delta(g0, Cm.graph_counts(solver))
            if path in ("small", "stream"):
                assert dg["captures"] == dg["replays"] == 0, dg
            elif call == 1:
                assert dg["replays"] == 1 and dg["captures"] == 0 and dg["drops"] == 0, dg
    finally:
        solver.set_tuning("small_grid", 1)
        solver.set_tuning("graph", 1)
        solver.set_tuning("team_launch", -1)
    for k in range(len(strikes)):
        p = O.make_params(m1, m2, Ns[k], Ts[k] / Ns[k], Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA,
                          variant, Cm.DIVS)
        Uo, lo, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k], U0[k])
        _assert_field(U[k], Uo)
        if variant == H.AM_DIV:
            assert np.abs(lam[k] - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


def test_device_memory_path_equals_host_path(solver):
    import torch
    m1, m2, N, strikes = 100, 50, 15, Cm.strikes_for(6)
    grids, U0, U_host, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU)
    dev = torch.device("cuda:0")
    gd = grids.to(dev)
    ws = H.DOWorkspace(len(strikes), (m1 + 1) * (m2 + 1), device=dev)
    ws.U.copy_(torch.from_numpy(U0))
    torch.cuda.synchronize()
    prices = solver.parallel_DO_solve(len(strikes), Cm.S_0, Cm.V_0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D,
                                      Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, gd, ws)
    assert prices.is_cuda
    assert np.array_equal(ws.U.cpu().numpy(), U_host)  # same kernels, same inputs: bit-identical
    i_s = grids_index = H.Grid(m1, 8 * strikes[0], Cm.S_0, strikes[0], strikes[0] / 5, m2, 5.0, Cm.V_0, 0.01)
    k = i_s.find_s_index(Cm.S_0) + i_s.find_v0_index(Cm.V_0) * (m1 + 1)
    assert prices.cpu().numpy()[0] == U_host[0, k]


def test_batch_composition_does_not_change_an_instance(solver):
    """Instances are independent (TeamPolicy league, device_solver.hpp:83-88): results must be
    bit-identical whatever else is in the batch and wherever the instance sits in it."""
    m1, m2, N = 128, 64, 10
    strikes = Cm.strikes_for(7)
    _, _, U_all, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU)
    perm = [3, 0, 6, 2]
    _, _, U_sub, _ = _hadi_solve(solver, m1, m2, N, [strikes[i] for i in perm], H.EU)
    for a, i in enumerate(perm):
        assert np.array_equal(U_sub[a], U_all[i])
    _, _, U_one, _ = _hadi_solve(solver, m1, m2, N, [strikes[5]], H.EU)
    assert np.array_equal(U_one[0], U_all[5])


def test_full_size_properties_config2(solver):
    """BASELINE config 2 at full size (512x256, 1000 steps, 4 instances): the oracle would need ~30 s
    per instance, so check (i) the recorded reference price, (ii) affine superposition of the Douglas
    map, S(U0 + W) - S(U0) = S(W) - S(0), which holds for ANY correct linear scheme and couples every
    row/column of the grid, (iii) discrete maximum-principle sanity 0 <= price <= S_0."""
    m1, m2, N = 512, 256, 1000
    K = 100.0
    grids1, U0 = _batch(m1, m2, [K])
    grids = H.GridViewsBatch([H.Grid(m1, 8 * K, Cm.S_0, K, K / 5, m2, 5.0, Cm.V_0, 5.0 / 500)] * 4)
    rng = np.random.default_rng(11)
    W = rng.standard_normal(U0.shape) * 3.0
    U = np.concatenate([U0, U0 + W, W, np.zeros_like(U0)])
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
    node = 181 + 78 * (m1 + 1)
    assert abs(U[0, node] - 8.8942192888223310) <= PRICE_ATOL
    lhs, rhs = U[1] - U[0], U[2] - U[3]
    assert np.abs(lhs - rhs).max() <= 1e-9 * max(1.0, np.abs(rhs).max())
    assert 0.0 <= U[0, node] <= Cm.S_0
    t = solver.timing()
    assert t["point_steps"] == 4 * 513 * 257 * 1000 and t["sweep_ms"] > 0


def test_error_conventions(solver):
    m1, m2, N = 40, 12, 3
    grids, U0 = _batch(m1, m2, [100.0])
    ws = H.DOWorkspace(1, (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    with pytest.raises(H.HadiError) as e:  # S_0 off-grid: the reference silently reads index -1
        solver.parallel_DO_solve(1, 101.2345, Cm.V_0, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO,
                                 Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, ws)
    assert e.value.status == 4
    g2, U2 = _batch(600, 528, [100.0])  # more than 16 chunks of 33 v-rows: the sequential column pass, Douglas / fp64 state only
    with pytest.raises(H.HadiError) as e:
        solver.CS_scheme(600, 528, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, g2, U2)
    assert e.value.status == 2
    with pytest.raises(H.HadiError) as e:
        solver.DO_timestepping(600, 528, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, g2, U2,
                               state_precision=H.STATE_FP32)
    assert e.value.status == 2
    for bad in ({"N_i": [0], "delta_t_i": [0.1]}, {"N_i": [3], "delta_t_i": [-0.1]}, {"N_i": [3], "delta_t_i": [float("nan")]}):
        with pytest.raises(H.HadiError) as e:  # per-instance overrides are validated entry by entry
            solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids,
                                   U0.copy(), per_instance=bad)
        assert e.value.status == 1
    with pytest.raises(ValueError):  # puts need their strikes
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids,
                               U0.copy(), option_type=H.PUT)
    with pytest.raises(H.HadiError):
        solver.set_tuning("no_such_key", 1)
    with pytest.raises(H.HadiError) as e:
        solver.DO_timestepping(m1, m2, 0, Cm.T, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U0.copy())
    assert e.value.status == 1
    with pytest.raises(ValueError):
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids,
                               U0[:, :-1].copy())
    # V_0 off-grid picks v-index 0 like the reference (grid_pod.hpp:76-87) -- no error
    ws.U[...] = U0
    p = solver.parallel_DO_solve(1, Cm.S_0, 0.0123, m1, m2, N, Cm.T, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO,
                                 Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, ws)
    i_s = H.Grid(m1, 800.0, Cm.S_0, 100.0, 20.0, m2, 5.0, Cm.V_0, 0.01).find_s_index(Cm.S_0)
    assert p[0] == ws.U[0, i_s]


def test_lm_calibration_trajectory_vs_oracle_driven_loop(solver):
    """N1: the LM loop (heston_calibration.cpp:204-417) on 12 strikes of the reference's 50x25x20
    calibration grid, libhadi solves vs the same loop driven by oracle solves.  Market = model prices at
    shifted parameters, so the loop must walk towards them.  Parameters agree to 1e-4 after 3 iterations
    (J^T J has cond ~1e9: Jacobian round-off of 1e-6 moves the weakly identified kappa in the 5th digit)."""
    m1, m2, N = 50, 25, 20
    strikes = [85.0 + 2.5 * k for k in range(12)]
    grids, U0 = _batch(m1, m2, strikes)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, -0.6, 0.45, 2.2, 0.06)
    market, _ = O.base_prices(p, Cm.S_0, 0.05, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    args = (Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0, m1, m2, N, Cm.THETA, grids, U0, market)
    got = H.calibrate_european(solver, *args, max_iter=3, tol=1e-12)
    want = H.calibrate_european(Cm.OracleSolver(), *args, max_iter=3, tol=1e-12)
    assert got["iterations"] == want["iterations"] == 3
    for hg, hw in zip(got["history"], want["history"]):
        assert abs(hg["error"] - hw["error"]) <= 1e-6 * max(1.0, hw["error"]) and hg["lambda"] == hw["lambda"]
    keys = ("kappa", "eta", "sigma", "rho", "v0")
    assert np.allclose([got[k] for k in keys], [want[k] for k in keys], rtol=1e-4, atol=1e-6)
    assert got["history"][-1]["error"] < 0.5 * got["history"][0]["error"]


def test_full_lm_calibration_reproduces_reference_run_on_gpu(solver):
    """N1 end to end on the device: the reference's test_calibration_european (60 strikes, 50x25x20, BS market at 20 %)
    run through libhadi lands on the recorded result -- 4 iterations, 1620 PDE solves, final error 0.0836893 and the
    five parameters (tests/golden).  Tolerance 1e-3 relative, not the 6 printed digits the serial
    oracle reproduces: the forward-difference Jacobian (eps = 1e-6) turns the 1e-15 round-off differences of the
    parallel line solves into 1e-9 in J, and four LM steps through J^T J with cond ~1e9 (kappa runs to 47.9, barely
    identified) carry that into the 5th digit of the final error and the 3rd-4th of kappa (observed 0.4e-3 .. 1.0e-3
    across kernel revisions that differ only in rounding), hence 3e-3 for kappa alone."""
    import test_oracle_golden as G
    g, args = G._reference_calibration_setup()
    res = H.calibrate_european(solver, *args, max_iter=15, tol=0.1)
    G.check_calibration_against_record(res, g, tol=1e-3, kappa_tol=3e-3)


REF_DIVS = ([0.2, 0.4, 0.6, 0.8], [0.10] * 4, [0.0005] * 4)  # heston_calibration.cpp:1090-1092


def _same_run(got, want):
    """Same LM path on libhadi and on the oracle.  The first iteration starts from identical parameters, so its
    error agrees to round-off; after that the forward-difference Jacobian (eps = 1e-6 -> 1e-9 noise in J) and the
    cond ~1e9 normal equations spread the two trajectories to ~1e-5 in the error and ~1e-3 in the barely
    identified kappa (the flat 20 % smile drives sigma to its floor), which is what the bounds below allow."""
    assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
    assert abs(got["history"][0]["error"] - want["history"][0]["error"]) <= 1e-9 * want["history"][0]["error"]
    for hg, hw in zip(got["history"], want["history"]):
        assert abs(hg["error"] - hw["error"]) <= 1e-4 * hw["error"] and hg["lambda"] == hw["lambda"]
    assert abs(got["kappa"] - want["kappa"]) <= 1e-2 * abs(want["kappa"])
    keys = ("eta", "sigma", "rho", "v0")
    assert np.allclose([got[k] for k in keys], [want[k] for k in keys], rtol=1e-3, atol=1e-6)
    assert np.allclose(got["model_prices"], want["model_prices"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("driver", ["american", "dividends", "american_dividends"])
def test_variant_calibration_drivers_vs_oracle_driven_loop(solver, driver):
    """test_calibration_american / _dividends / _american_dividends (heston_calibration.cpp:515-2160) on their own
    setups: the same host loop over libhadi launchers and over oracle launchers must take the same path."""
    m1, m2, N = 50, 25, 20
    if driver == "american":
        strikes = [Cm.S_0 * 0.55 + i for i in range(10)]
        market = H.market.generate_market_data(Cm.S_0, Cm.T, Cm.R_D, strikes)
        extra = ()
    else:
        strikes = [Cm.S_0 * 0.7 + i for i in range(60)]
        market = H.market.generate_market_data_with_dividends(Cm.S_0, Cm.T, Cm.R_D, strikes, *REF_DIVS)
        extra = (H.Dividends(*REF_DIVS),)
    grids, U0 = _batch(m1, m2, strikes)
    args = (Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0, m1, m2, N, Cm.THETA, grids, U0,
            market) + extra
    fn = getattr(H, "calibrate_" + driver)
    _same_run(fn(solver, *args), fn(Cm.OracleSolver(), *args))


def test_multi_maturity_calibration_drivers_vs_oracle_driven_loop(solver):
    """test_calibration_european_multi_maturity (heston_calibration.cpp:2428-2933; 10 maturities x 20 strikes, BS market)
    and test_calibration_american_divident_multi_maturity (:3245-3820; 3 maturities x 60 strikes, market generated by
    the model itself at kappa=3, eta=0.1, sigma=0.05, rho=0.2, v0=0.06) through the multi-maturity launchers."""
    m1, m2 = 50, 25
    start = (Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0)
    mats = [1.0 + i * 0.25 if i < 8 else 3.0 + (i - 8) * 0.5 for i in range(10)]
    pts = H.make_calibration_points([Cm.S_0 * 0.95 + 0.5 * i for i in range(20)], mats)
    ks = [p.strike for p in pts]
    grids, U0 = _batch(m1, m2, ks)
    market = np.array([H.market.call_price(Cm.S_0, p.strike, Cm.R_D, 0.2, p.maturity) for p in pts])
    args = (Cm.S_0, Cm.R_D, Cm.R_F) + start + (m1, m2, Cm.THETA, pts, grids, U0, market)
    _same_run(H.calibrate_european_multi_maturity(solver, *args),
              H.calibrate_european_multi_maturity(Cm.OracleSolver(), *args))

    pts = H.make_calibration_points([Cm.S_0 * 0.7 + i for i in range(60)], [1.0, 1.5, 2.0])
    ks = [p.strike for p in pts]
    grids, U0 = _batch(m1, m2, ks)
    div = H.Dividends(*REF_DIVS)
    ws = H.DOWorkspace(len(pts), (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    market = solver.compute_base_prices_multi_maturity_american_dividends(
        Cm.S_0, 0.06, Cm.R_D, Cm.R_F, 0.2, 0.05, 3.0, 0.1, m1, m2, (m1 + 1) * (m2 + 1), Cm.THETA, pts, len(pts), grids,
        U0, ws, div)
    ws.U[...] = U0
    market_o = Cm.OracleSolver().compute_base_prices_multi_maturity_american_dividends(
        Cm.S_0, 0.06, Cm.R_D, Cm.R_F, 0.2, 0.05, 3.0, 0.1, m1, m2, (m1 + 1) * (m2 + 1), Cm.THETA, pts, len(pts), grids,
        U0, ws, div)
    assert np.abs(market - market_o).max() <= PRICE_ATOL
    args = (Cm.S_0, Cm.R_D, Cm.R_F) + start + (m1, m2, Cm.THETA, pts, grids, U0, market_o, div)
    _same_run(H.calibrate_american_dividends_multi_maturity(solver, *args, max_iter=4),
              H.calibrate_american_dividends_multi_maturity(Cm.OracleSolver(), *args, max_iter=4))


@pytest.mark.parametrize("variant,name", [(H.EU, "EU"), (H.AM, "AM"), (H.AM_DIV, "AM_DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(512, 256, 8, 2), (300, 140, 5, 1), (260, 200, 4, 3), (400, 33, 6, 2),
                                      (256, 128, 6, 2), (200, 100, 5, 2), (100, 50, 4, 3)])
def test_strip_row_pass_vs_oracle(solver, forced_strips, variant, name, m1, m2, N, n):
    """The barrier-free strip row pass (2, 4 or 8 nodes per lane) is only chosen for large batches; force it on small ones so
    that every strip geometry (short strips, ragged last strip, one block or several per instance) meets the oracle."""
    strikes = Cm.strikes_for(n)
    solver.set_tuning("american_p", 0)  # the P representation runs on the shared-ring kernel; here: the strips' explicit path
    try:
        grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, r_f=0.01, want_lambda=(variant != H.EU))
    finally:
        solver.set_tuning("american_p", 1)
    assert "hadi_pass_a_strip" in solver.describe_last_sweep()
    p = Cm.oracle_params(m1, m2, N, name, r_f=0.01)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    if lam is not None:
        assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("variant,name,american_p", [(H.EU, "EU", 1), (H.DIV, "DIV", 1), (H.AM, "AM", 0), (H.AM, "AM", 1), (H.AM_DIV, "AM_DIV", 1)])
@pytest.mark.parametrize("m1,m2,N,n", [(256, 128, 25, 3), (200, 100, 6, 2), (130, 20, 5, 2), (180, 33, 7, 1), (256, 70, 6, 5)])
def test_pair_strips_vs_oracle(solver, forced_strips, variant, name, american_p, m1, m2, N, n):
    """128 < m1 <= 256: hadi_pass_a_pairs -- two strips per wavefront on the 8-nodes-per-lane arithmetic (lanes 0..31 / 32..63),
    chosen by itself for batches that fill the GPU (config 3: test_config3_batch_geometry_field_vs_oracle), forced here on
    small ones: strips of equal and unequal length, an empty second strip (130x20: 21 rows), the b2 row in either half,
    dividend steps in between (N = 25), the explicit (U, lambda_bar) pair and the P representation; U and lambda_bar
    of every instance against the oracle."""
    strikes = Cm.strikes_for(n)
    solver.set_tuning("pair_strips", 1)
    solver.set_tuning("american_p", american_p)
    try:
        grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, r_f=0.01, want_lambda=(variant in (H.AM, H.AM_DIV)))
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("pair_strips", -1)
        solver.set_tuning("american_p", 1)
    assert "hadi_pass_a_pairs<%s>" % ("EU" if variant in (H.EU, H.DIV) else "AM-P" if american_p else "AM") in d, d
    p = Cm.oracle_params(m1, m2, N, name, r_f=0.01)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    if lam is not None:
        assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("variant,name", [(H.AM, "AM"), (H.AM_DIV, "AM_DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(512, 256, 12, 2), (300, 140, 25, 2), (256, 128, 25, 3), (128, 64, 10, 2)])
def test_strip_row_pass_with_the_p_representation(solver, forced_strips, variant, name, m1, m2, N, n):
    """American sweeps in the P representation on the barrier-free strips (chosen by itself for large batches at 8 and 2
    nodes per lane; forced here): U = max(P, U_0) rebuilt on the register window and the ring rows, lambda_bar from the
    raw P of row j, payoff row in LDS.  N = 25 puts dividend steps (explicit pair, materialise / dematerialise) in between."""
    strikes = Cm.strikes_for(n)
    grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, variant, r_f=0.01, want_lambda=True)
    d = solver.describe_last_sweep()
    assert "hadi_pass_a_strip" in d and "AM-P" in d
    p = Cm.oracle_params(m1, m2, N, name, r_f=0.01)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("theta", [0.0, 0.5, 1.0])
def test_strip_row_pass_theta_range(solver, forced_strips, theta):
    """The strip kernel forms I - theta dt A1 directly and rebuilds the explicit A1 action from it with the factor
    (1 - theta) / theta: theta = 1 (factor 0) and theta = 0.5 must meet the oracle, and theta = 0 -- where that factor does
    not exist -- must be kept off the strip kernel by the host even when strips are forced."""
    m1, m2, N, n = 300, 140, 6, 2
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    dt = Cm.T / (50 * N) if theta > 0 else 1e-6  # (the explicit scheme is only stable for tiny steps on this grid)
    solver.DO_timestepping(m1, m2, N, dt, theta, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
    assert ("hadi_pass_a_strip" in solver.describe_last_sweep()) == (theta > 0)
    p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU, None)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("variant,name", [(H.EU, "EU"), (H.DIV, "DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(600, 40, 5, 2), (1024, 64, 4, 2), (700, 300, 4, 2), (1024, 512, 3, 1), (530, 37, 24, 3)])
def test_paired_strip_row_pass_vs_oracle(solver, forced_strips, fp32, variant, name, m1, m2, N, n):
    """512 < m1 <= 1024 on barrier-free strips: a pair of wavefronts per strip, half a row each (own LDS-DMA pieces and
    counted waits, split tridiagonal solve with the 2x2 exchange and a pair rendezvous per row, the partner's boundary node
    read from the partner's half of the ring).  Chosen by itself for large batches (config 5); forced here so that short,
    ragged, ascending and descending strips, the 3-slot ring (fp64 state) and the 4-slot ring of floats meet the oracle."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    div = H.Dividends(*Cm.DIVS) if variant == H.DIV else None
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                           variant=variant, dividends=div, state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64)
    assert ("hadi_pass_a_strip<8,EU,float,2>" if fp32 else "hadi_pass_a_strip<8,EU,double,2>") in solver.describe_last_sweep()
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA,
                      O.DIV if variant == H.DIV else O.EU, Cm.DIVS if variant == H.DIV else None, state_fp32=1 if fp32 else 0)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    if fp32:
        _assert_field(U, Uo, rtol=2e-7 * N)
    else:
        _assert_field(U, Uo)


@pytest.mark.parametrize("m1,m2,N", [(600, 40, 5), (700, 300, 4), (1024, 512, 3)])
@pytest.mark.parametrize("variant", ["AM", "AM_DIV"])
@pytest.mark.parametrize("american_p", [1, 0])
def test_american_sweeps_of_wide_grids_on_paired_strips(solver, forced_strips, m1, m2, N, variant, american_p):
    """512 < m1 <= 1024, American and American-with-dividends sweeps on the paired strips (round 3; until then they fell back
    to the shared ring): the P representation (u0 carried raw, U = max(P, U_0) rebuilt inside the step, explicit steps on the
    first step and on dividend dates) and the explicit (U, lambda_bar) pair; U and lambda_bar of every instance against the
    oracle (device_solver.hpp:274-374, 650-942)."""
    n = 2
    strikes = Cm.strikes_for(n)
    solver.set_tuning("american_p", american_p)
    try:
        grids, U0, U, lam = _hadi_solve(solver, m1, m2, N, strikes, getattr(H, variant), r_f=0.01, want_lambda=True)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("american_p", 1)
    assert ("hadi_pass_a_strip<8,AM-P,double,2>" if american_p else "hadi_pass_a_strip<8,AM,double,2>") in d, d
    p = Cm.oracle_params(m1, m2, N, variant, r_f=0.01)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    _assert_field(U, Uo)
    assert np.abs(lam - lo).max() <= 1e-8 * max(1.0, np.abs(lo).max())


@pytest.mark.parametrize("m1,m2,N,n", [(100, 50, 5, 3), (256, 128, 5, 2), (400, 131, 5, 2), (512, 256, 6, 2), (600, 40, 5, 2), (1024, 100, 4, 1)])
def test_craig_sneyd_on_strips_vs_oracle_ring_and_full_drains(solver, strict_solver, forced_strips, m1, m2, N, n):
    """Round 4: predictor and corrector row passes of a Craig-Sneyd step on the barrier-free strips (2, 4, 8 nodes per lane,
    paired strips above 512 s-intervals).  Full field against the oracle; against the shared-ring kernels (tuning key
    `cs_strips` = 0: the path of rounds 2 - 3) to round-off; and bit for bit against libhadi_strict.so, whose waits drain
    everything."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids)
    U = U0.copy()
    solver.CS_scheme(*args, U)
    d = solver.describe_last_sweep()
    assert ("hadi_pass_a_strip<8,EU,double,2,CS>" if m1 > 512 else "hadi_pass_a_strip<%d,EU,double,1,CS>" % (2 if m1 <= 128 else 4 if m1 <= 256 else 8)) in d, d
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU, None, scheme=1)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)
    solver.set_tuning("cs_strips", 0)
    try:
        Ur = U0.copy()
        solver.CS_scheme(*args, Ur)
        assert "strip" not in solver.describe_last_sweep()
    finally:
        solver.set_tuning("cs_strips", 1)
    assert np.abs(U - Ur).max() <= 1e-11 * np.abs(Uo).max()
    strict_solver.set_tuning("strip", 1)
    try:
        Us = U0.copy()
        strict_solver.CS_scheme(*args, Us)
        assert strict_solver.describe_last_sweep() == d
    finally:
        strict_solver.set_tuning("strip", -1)
    assert np.array_equal(U, Us)


LOAD_CASES = [  # (m1, m2, N, n, variant, tuning, fp32, kernel expected in the description[, kernel that must NOT be in it])
    # config 2 on the streaming strip kernel at the headline geometry (it serves every remainder sub-batch, profiled run and pinned
    # geometry; the default path of this batch is the resident sweep: the last case)
    (512, 256, 20, 256, H.EU, {"resident_sweep": 0}, False, "hadi_pass_a_strip<8,EU>", "hadi_sweep_resident"),
    (512, 256, 12, 256, H.AM, {}, False, "hadi_pass_a_strip<8,AM-P>"),                  # P representation on strips
    (512, 256, 12, 256, H.AM, {"american_p": 0}, False, "hadi_pass_a_strip<8,AM>"),     # explicit (U, lambda_bar) pair
    (512, 256, 12, 160, H.EU, {}, False, "two streams"),                               # two half-batches side by side
    (512, 256, 12, 48, H.EU, {"strip": 0}, False, "hadi_pass_a<8,1"),                   # shared ring
    (256, 128, 25, 512, H.AM_DIV, {}, False, "hadi_pass_a_pairs<AM-P>"),                # config 3 as benchmarked
    (256, 128, 12, 300, H.EU, {"strip": 1, "pair_strips": 0}, False, "hadi_pass_a_strip<4,EU>"),
    (128, 64, 12, 1100, H.EU, {}, False, "hadi_pass_a_strip<2,EU>"),
    (1024, 512, 8, 64, H.EU, {}, False, "hadi_pass_a_strip<8,EU,double,2>"),            # config 5, fp64 state
    (1024, 512, 8, 64, H.EU, {}, True, "hadi_pass_a_strip<8,EU,float,2>"),              # config 5, fp32 state
    (1024, 512, 6, 64, H.AM, {}, False, "hadi_pass_a_strip<8,AM-P,double,2>"),
    (512, 256, 20, 256, H.EU, {}, False, "hadi_sweep_resident<8>"),                     # config 2 as benchmarked: the resident sweep
]


def _load_key(m1, m2, N, n, variant, tuning, fp32, kernel):
    return (m1, m2, N, n, variant, tuple(sorted(tuning.items())), fp32, kernel)


LOAD_ABSENT = {_load_key(*c[:8]): c[8] for c in LOAD_CASES if len(c) > 8}  # (the optional ninth field)


@pytest.mark.parametrize("m1,m2,N,n,variant,tuning,fp32,kernel", [c[:8] for c in LOAD_CASES])
def test_counted_waits_under_load_equal_full_drains(solver, strict_solver, m1, m2, N, n, variant, tuning, fp32, kernel):
    """test_counted_vmcnt_waits_equal_full_drains (below) compares the two builds on two or three instances -- where every
    load has landed long before it is waited for.  The defect of round 4's first strip corrector only showed with every CU
    streaming; so the same comparison at the benchmarked batch geometries: every row-pass family with counted waits, bit for
    bit against the build that drains everything."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    res = []
    absent = LOAD_ABSENT.get(_load_key(m1, m2, N, n, variant, tuning, fp32, kernel))
    reset = {"strip": -1, "american_p": 1, "pair_strips": -1, "resident_sweep": -1}
    for sv in (solver, strict_solver):
        for k, v in tuning.items():
            sv.set_tuning(k, v)
        try:
            U, lam = U0.copy(), np.zeros_like(U0)
            american = variant in (H.AM, H.AM_DIV)
            sv.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               variant=variant, U_0=U0, lambda_bar=lam if american else None,
                               dividends=H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None,
                               state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64)
        finally:
            for k in tuning:
                sv.set_tuning(k, reset[k])
        res.append((U, lam, sv.describe_last_sweep()))
    assert kernel in res[0][2], res[0][2]
    assert absent is None or absent not in res[0][2], res[0][2]
    assert res[0][2] == res[1][2]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][0]).all()


def test_craig_sneyd_on_strips_under_load_equals_full_drains(solver, strict_solver):
    """Counted waits are a statement about ISSUE ORDER; whether a wrong one shows depends on how late the memory system answers.
    A batch that fills the chip (256 instances of 512x256: the plan picks the strips by itself) over 60 time steps -- 120
    predictor and 120 corrector launches with every CU streaming -- must equal the build whose waits drain everything, bit for
    bit, on every instance.  (This test was written before the first strip corrector was trusted, and failed: that version
    loaded its R1 / C2 rows from inline asm and the compiler moved copies of the in-flight registers above the wait -- every
    small test passed.  DESIGN.md section 4.2.)"""
    m1, m2, N, n = 512, 256, 60, 256
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids)
    U, Us = U0.copy(), U0.copy()
    solver.CS_scheme(*args, U)
    d = solver.describe_last_sweep()
    assert "hadi_pass_a_strip<8,EU,double,1,CS>" in d, d
    strict_solver.CS_scheme(*args, Us)
    assert strict_solver.describe_last_sweep() == d
    assert np.array_equal(U, Us)
    assert np.isfinite(U).all() and np.abs(U).max() < 1e4


def test_strips_chosen_by_themselves_at_two_nodes_per_lane(solver):
    """64 < m1 <= 128 with several blocks per CU: the plan picks 4-strip blocks on its own (hadi_plan.h); 1100 instances
    of 128x64, a few steps, against the oracle."""
    m1, m2, N, n = 128, 64, 4, 1100
    strikes = Cm.strikes_for(n)
    grids, U0, U, _ = _hadi_solve(solver, m1, m2, N, strikes, H.EU)
    assert "hadi_pass_a_strip<2,EU>" in solver.describe_last_sweep()
    p = Cm.oracle_params(m1, m2, N, "EU")
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


def test_forced_strips_leave_the_fp32_state_of_narrow_grids_on_the_ring_kernel(solver, forced_strips):
    """The float strip kernel exists at 8 nodes per lane only: with strips forced (or auto-selected at 2 nodes per lane) a
    narrower grid with the fp32 state must take the shared-ring float kernel, not a mismatched strip launch."""
    m1, m2, N, n = 128, 64, 6, 3
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                           state_precision=H.STATE_FP32)
    d = solver.describe_last_sweep()
    assert "float" in d and "strip" not in d
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU, None, state_fp32=1)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo, rtol=2e-7 * N)


@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 20, 3), (128, 64, 10, 2), (256, 128, 12, 3), (512, 256, 8, 2),
                                      (1024, 512, 4, 1), (700, 300, 4, 2)])
def test_fp32_state_sweep_vs_oracle(solver, m1, m2, N, n):
    """BASELINE config 5 ("mixed-precision fp32 ADI sweep with fp64 tridiag pivots"): U and the A2 right-hand side are
    stored as fp32 between the passes, all arithmetic is fp64.  Not a reference feature -- the checker is the oracle
    with the same two roundings per step; an fp64 last-bit difference before a store can flip a float rounding
    (6e-8 relative), hence 2e-7 per step.  Against the fp64 sweep the price moves by a few 1e-6 relative."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    if m1 == 512:
        solver.set_tuning("strip", 1)  # the strip row pass with a ring of floats (chosen by itself for large batches)
    try:
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               state_precision=H.STATE_FP32)
    finally:
        solver.set_tuning("strip", -1)
    assert "float" in solver.describe_last_sweep() and (("strip" in solver.describe_last_sweep()) == (m1 == 512))
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=0.01)
    p.state_fp32 = 1
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo, rtol=2e-7 * N)
    p.state_fp32 = 0
    U64, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, U64, rtol=2e-6)


@pytest.mark.parametrize("m1,m2,N,n,strip", [(128, 64, 24, 2, -1), (512, 256, 24, 2, 1), (700, 300, 22, 1, -1)])
def test_fp32_state_with_dividends_vs_oracle(solver, m1, m2, N, n, strip):
    """fp32 state + discrete dividends: on dividend steps the state is widened, the jump (device_solver.hpp:448-504) runs
    on the fp64 packed array, and the result is rounded again -- the oracle does the same."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    solver.set_tuning("strip", strip)
    try:
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               variant=H.DIV, dividends=H.Dividends(*Cm.DIVS), state_precision=H.STATE_FP32)
    finally:
        solver.set_tuning("strip", -1)
    assert "float" in solver.describe_last_sweep()
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.DIV, Cm.DIVS, state_fp32=1)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo, rtol=2e-7 * N)


def test_fp32_state_price_error_is_1e_6_to_1e_5(solver):
    """What the fp32 state costs: every step rounds U and the A2 right-hand side to 24 bits (6e-8 relative); the
    perturbations add up like a random walk, damped by the diffusion.  Price difference to the fp64 sweep on the 512x256
    grid for N = 125 .. 2000 (T = 1): one realisation per N, erratic, between 1e-7 and 1.3e-5 (observed 1.3e-5, 3.5e-6,
    2.1e-6, 1.1e-7, 1.0e-5) -- this mode does NOT guarantee a 1e-6 price tolerance (hadi.h says so).  No
    compensated variant is offered: keeping the lost bits costs as many bytes as the fp64 state (fp32 value + fp32 error
    term = 8 B), a 6-byte split format would save a quarter of the column pass's traffic only, and the row pass is
    instruction-bound either way."""
    m1, m2, K = 512, 256, 100.0
    Ns = [125, 250, 500, 1000, 2000]
    grids = H.GridViewsBatch([H.Grid(m1, 8 * K, Cm.S_0, K, K / 5, m2, 5.0, Cm.V_0, 5.0 / 500)] * len(Ns))
    U0 = grids.call_payoff([K] * len(Ns))
    per = {"N_i": Ns, "delta_t_i": [Cm.T / N for N in Ns]}
    out = []
    for prec in (H.STATE_FP64, H.STATE_FP32):
        U = U0.copy()
        solver.DO_timestepping(m1, m2, 1, 1.0, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               per_instance=per, state_precision=prec)
        out.append(U.copy())
    node = 181 + 78 * (m1 + 1)
    err = np.abs(out[1][:, node] - out[0][:, node])
    print("fp32-state price error vs N:", dict(zip(Ns, err)))
    assert abs(out[0][3, node] - 8.8942192888223310) < 1e-9
    assert err.max() < 5e-5 and err.max() > 1e-6
    field = np.abs(out[1] - out[0]).max(axis=1) / np.abs(out[0]).max(axis=1)
    print("fp32-state field error (relative to max|U|) vs N:", dict(zip(Ns, field)))
    # the FIELD error grows faster than a random walk (1.5e-7, 3.4e-7, 2.5e-6, 5.4e-6, 1.4e-5 of max|U| for the five N):
    # where the per-step increment falls below half an fp32 ulp of the value it is absorbed by the rounding (stagnation)
    assert field.max() < 5e-5 and field[0] < 1e-6


def test_fp32_state_restrictions(solver):
    m1, m2, N = 64, 32, 4
    grids, U0 = _batch(m1, m2, [100.0])
    for kw in ({"variant": H.AM, "U_0": U0}, {"scheme": 1}):
        with pytest.raises(H.HadiError) as e:
            solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids,
                                   U0.copy(), state_precision=H.STATE_FP32, **kw)
        assert e.value.status == 2  # HADI_ERR_UNSUPPORTED


@pytest.mark.parametrize("put", [False, True])
@pytest.mark.parametrize("variant,name", [(H.EU, "EU"), (H.DIV, "DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 24, 5), (25, 20, 20, 3), (100, 25, 6, 2), (128, 26, 5, 2), (64, 32, 7, 3), (20, 25, 9, 2), (65, 8, 24, 4)])
def test_small_grid_sequential_kernel_vs_oracle(solver, put, variant, name, m1, m2, N, n):
    """hadi_small_seq_kernel (one wavefront per instance; lane <-> v-row in the row pass, lane <-> s-column in the column
    pass) on the LDS-resident shapes: one and two nodes per packed lane, two and three column rounds (m1 > 63), m2 > m1, the
    full 33 v-rows, dividends, put boundary data, r_f != 0 -- full field against the oracle."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    if put:
        U0 = grids.put_payoff(strikes)
    U = U0.copy()
    div = H.Dividends(*Cm.DIVS) if variant == H.DIV else None
    solver.set_tuning("small_seq", 1)  # (chosen by itself for batches of more instances than CUs)
    try:
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               variant=variant, dividends=div, option_type=H.PUT if put else H.CALL, strikes=strikes if put else None)
    finally:
        solver.set_tuning("small_seq", -1)
    assert "hadi_small_seq_kernel" in solver.describe_last_sweep()
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA,
                      O.DIV if variant == H.DIV else O.EU, Cm.DIVS if variant == H.DIV else None,
                      option_type=O.PUT if put else O.CALL, strikes=np.array(strikes) if put else None)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(U, Uo)


@pytest.mark.parametrize("put", [False, True])
@pytest.mark.parametrize("variant,name", [(H.EU, "EU"), (H.DIV, "DIV")])
@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 24, 5), (25, 20, 20, 3), (100, 25, 6, 2), (128, 26, 5, 7), (64, 31, 7, 4), (20, 25, 9, 1), (65, 8, 24, 6)])
def test_small_grid_two_instances_per_wavefront_vs_oracle(solver, put, variant, name, m1, m2, N, n):
    """hadi_small_seq2_kernel: lanes 0..31 / 32..63 walk the v-rows of two instances through one instruction stream (chosen
    by itself for batches of more than two instances per CU; forced here): even and odd batches (the last wavefront carries
    one instance), a single instance, one and two nodes per packed lane, dividends, put data, r_f != 0 -- full field against
    the oracle, and BIT-identical to the one-instance-per-wavefront kernel (same arithmetic, operation by operation)."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    if put:
        U0 = grids.put_payoff(strikes)
    div = H.Dividends(*Cm.DIVS) if variant == H.DIV else None
    out = {}
    solver.set_tuning("small_seq", 1)
    try:
        for pairs in (1, 0):
            solver.set_tuning("small_pairs", pairs)
            U = U0.copy()
            solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                                   variant=variant, dividends=div, option_type=H.PUT if put else H.CALL, strikes=strikes if put else None)
            assert ("hadi_small_seq2_kernel" if pairs else "hadi_small_seq_kernel") in solver.describe_last_sweep()
            out[pairs] = U
    finally:
        solver.set_tuning("small_seq", -1)
        solver.set_tuning("small_pairs", -1)
    assert np.array_equal(out[1], out[0])
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA,
                      O.DIV if variant == H.DIV else O.EU, Cm.DIVS if variant == H.DIV else None,
                      option_type=O.PUT if put else O.CALL, strikes=np.array(strikes) if put else None)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    _assert_field(out[1], Uo)


@pytest.mark.parametrize("seq", [1, 0])
def test_small_grid_kernel_on_a_batch_larger_than_two_per_cu(solver, seq):
    """A batch of several instances per CU with per-instance maturities (dispatch order: longest time loops first) on both
    LDS-resident kernels: the one-wavefront-per-instance sequential kernel (default for European / dividend sweeps) and the
    block-per-instance kernel (more than 2 instances per CU -> 4 wavefronts per instance, its throughput shape)."""
    m1, m2, n = 50, 25, 640
    strikes = Cm.strikes_for(n)
    Ns = [4 + (k % 5) for k in range(n)]
    per = {"N_i": Ns, "delta_t_i": [0.5 / N for N in Ns]}
    grids, U0 = _batch(m1, m2, strikes)
    U = U0.copy()
    solver.set_tuning("small_seq", seq)
    try:
        solver.DO_timestepping(m1, m2, 1, 1.0, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               per_instance=per)
    finally:
        solver.set_tuning("small_seq", -1)
    # (more than two instances per CU: the sequential kernel runs two instances per wavefront, each stopping at its own N)
    assert ("hadi_small_seq2_kernel<1>" if seq else "hadi_small_kernel<1,4,EU>") in solver.describe_last_sweep()
    for N in sorted(set(Ns)):
        rows = np.array([k for k in range(n) if Ns[k] == N])
        p = O.make_params(m1, m2, N, 0.5 / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
        Uo, _, _ = O.solve_batch(p, grids.Vec_s[rows], grids.Vec_v[rows], grids.Delta_s[rows], grids.Delta_v[rows], U0[rows])
        _assert_field(U[rows], Uo)


@pytest.mark.parametrize("m1,m2,N,n,variant,fp32", [(1024, 512, 3, 6, "EU", False), (1024, 512, 3, 5, "EU", True), (300, 270, 4, 3, "DIV", False),
                                                     (600, 400, 3, 40, "EU", False), (512, 256, 4, 20, "EU", False), (512, 256, 4, 9, "AM", False),
                                                     (256, 128, 24, 11, "AM_DIV", False)])
def test_column_pass_alternatives_prefetch_and_interleaved_tiles(solver, m1, m2, N, n, variant, fp32):
    """The two opt-in alternatives of the column pass (round 4, both measured neutral: profiles/r04_colpass_ab.txt): "col_prefetch"
    -- hadi_pass_b2, European sweeps of 9 .. 16 chunks with the first 12 (fp32 state: 24) rows of the next tile prefetched into
    LDS by LDS-DMA and ONE exchange buffer -- and "tile_interleave" -- the blocks of an instance take their full column tiles
    interleaved, on every column kernel.  Same arithmetic on the same data: bit-identical to the default path, which is
    checked against the oracle."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    v = getattr(H, variant)
    american = v in (H.AM, H.AM_DIV)
    res = {}
    for alt in (0, 1):
        solver.set_tuning("col_prefetch", alt)
        solver.set_tuning("tile_interleave", alt)
        try:
            U, lam = U0.copy(), np.zeros_like(U0)
            solver.DO_timestepping(m1, m2, N, Cm.T / 500, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U, variant=v,
                                   U_0=U0, lambda_bar=lam if american else None,
                                   dividends=H.Dividends(*Cm.DIVS) if v in (H.DIV, H.AM_DIV) else None,
                                   state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64)
            res[alt] = (U, lam, solver.describe_last_sweep())
        finally:
            solver.set_tuning("col_prefetch", 0)
            solver.set_tuning("tile_interleave", 0)
    assert ("hadi_pass_b2" in res[1][2]) == (m2 > 263 and not american), res[1][2]
    assert "hadi_pass_b2" not in res[0][2]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    p = O.make_params(m1, m2, N, Cm.T / 500, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, getattr(O, variant),
                      Cm.DIVS if v in (H.DIV, H.AM_DIV) else None, state_fp32=1 if fp32 else 0)
    rows = np.array(sorted({0, n // 2, n - 1}))
    Uo, _, _ = O.solve_batch(p, grids.Vec_s[rows], grids.Vec_v[rows], grids.Delta_s[rows], grids.Delta_v[rows], U0[rows], U0[rows])
    assert np.abs(res[1][0][rows] - Uo).max() <= (2e-7 * N if fp32 else FIELD_RTOL) * np.abs(Uo).max()


def test_describe_last_sweep_names_the_kernels(solver):
    _hadi_solve(solver, 50, 25, 4, [100.0], H.EU)
    assert "hadi_small_kernel<1,8,EU>" in solver.describe_last_sweep()
    _hadi_solve(solver, 50, 25, 2, Cm.strikes_for(400), H.EU)    # more instances than CUs: one wavefront per instance
    assert "hadi_small_seq_kernel<1>" in solver.describe_last_sweep()
    _hadi_solve(solver, 50, 25, 2, Cm.strikes_for(1100), H.EU)   # 2 .. 4.5 per CU: two instances per wavefront
    assert "hadi_small_seq2_kernel<1>" in solver.describe_last_sweep()
    _hadi_solve(solver, 50, 25, 2, Cm.strikes_for(1600), H.EU)   # the LDS is full either way: one wavefront per instance
    assert "hadi_small_seq_kernel<1>" in solver.describe_last_sweep()
    _hadi_solve(solver, 50, 25, 2, Cm.strikes_for(1100), H.AM)
    assert "hadi_small_kernel<1,4,AM>" in solver.describe_last_sweep()
    _hadi_solve(solver, 128, 64, 2, [100.0], H.AM)
    d = solver.describe_last_sweep()
    assert "hadi_pass_a<2,1" in d and "AM-P" in d and "hadi_pass_b<8,AM-P>" in d
    _hadi_solve(solver, 512, 256, 2, Cm.strikes_for(256), H.EU)   # enough rows per wavefront for the strip kernel
    d = solver.describe_last_sweep()
    assert "hadi_pass_a_strip<8,EU> (strips of 33 rows)" in d and "hadi_pass_b<8,EU>" in d
    _hadi_solve(solver, 1024, 512, 2, [100.0], H.EU)
    assert "hadi_pass_b1<16,EU>" in solver.describe_last_sweep()


def test_profiling_reports_kernel_times(solver):
    m1, m2, N = 128, 64, 20
    solver.set_profiling(True)
    try:
        _hadi_solve(solver, m1, m2, N, Cm.strikes_for(8), H.EU)
        t = solver.timing()
    finally:
        solver.set_profiling(False)
    assert t["pass_a_launches"] == N and t["pass_b_launches"] == N
    assert 0 < t["pass_a_ms"] <= t["sweep_ms"] * 1.05 and 0 < t["pass_b_ms"] <= t["sweep_ms"] * 1.05


STRICT_CASES = [
    # m1, m2, N, n, variant, tuning, fp32      every kernel that waits on a hand-counted vmcnt
    (512, 256, 6, 2, H.EU, {"strip": 1}, False),
    (512, 256, 6, 2, H.AM, {"strip": 1, "american_p": 0}, False),
    (512, 256, 6, 2, H.AM, {"strip": 1}, False),
    (512, 256, 6, 2, H.EU, {"strip": 1}, True),
    (256, 128, 6, 3, H.AM_DIV, {"strip": 1}, False),
    (128, 64, 6, 3, H.EU, {"strip": 1}, False),
    (512, 256, 6, 2, H.EU, {"strip": 0}, False),
    (200, 100, 6, 2, H.AM, {"strip": 0}, False),
    (100, 50, 6, 2, H.EU, {"strip": 0, "small_grid": 0}, False),
    (700, 300, 4, 1, H.EU, {}, True),
    (700, 300, 4, 1, H.EU, {"strip": 1}, False),   # paired strips, 3-slot ring
    (1024, 100, 4, 2, H.EU, {"strip": 1}, True),   # paired strips, 4-slot ring of floats
    (1024, 512, 3, 1, H.EU, {"strip": 1}, False),
    (700, 300, 4, 2, H.AM, {"strip": 1, "american_p": 0}, False),   # paired strips, explicit (U, lambda_bar) pair
    (700, 300, 4, 2, H.AM_DIV, {"strip": 1}, False),                # paired strips, P representation (+ explicit steps)
    (1024, 512, 3, 1, H.AM, {"strip": 1}, False),
    (256, 128, 6, 3, H.EU, {"strip": 1, "pair_strips": 1}, False),        # two strips per wavefront (hadi_pass_a_pairs)
    (256, 128, 25, 3, H.AM_DIV, {"strip": 1, "pair_strips": 1}, False),   # ... P representation with explicit steps in between
    (200, 100, 6, 2, H.AM, {"strip": 1, "pair_strips": 1, "american_p": 0}, False),
]


@pytest.fixture(scope="module")
def strict_solver():
    """libhadi_strict.so: the same sources with every counted `s_waitcnt vmcnt(n)` replaced by a full drain."""
    import __graft_entry__ as G
    s = H.HestonADI(0, lib_path=G.build_libhadi_strict())
    yield s
    s.close()


@pytest.mark.parametrize("m1,m2,N,n,variant,tuning,fp32", STRICT_CASES)
def test_counted_vmcnt_waits_equal_full_drains(solver, strict_solver, m1, m2, N, n, variant, tuning, fp32):
    """The LDS-DMA prefetch of the row passes is retired by hand-counted waits (issue-order bookkeeping of DMA pieces and
    result stores).  An under-count would read ring rows that have not landed -- silently.  The checking build waits for
    everything; both builds must agree bit for bit."""
    strikes = Cm.strikes_for(n)
    grids, U0 = _batch(m1, m2, strikes)
    res = []
    for sv in (solver, strict_solver):
        for k, v in tuning.items():
            sv.set_tuning(k, v)
        try:
            U, lam = U0.copy(), np.zeros_like(U0)
            american = variant in (H.AM, H.AM_DIV)
            sv.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               variant=variant, U_0=U0, lambda_bar=lam if american else None,
                               dividends=H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None,
                               state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64)
        finally:
            for k in tuning:
                sv.set_tuning(k, {"strip": -1, "small_grid": 1, "american_p": 1, "pair_strips": -1}[k])
        res.append((U, lam, sv.describe_last_sweep()))
    assert res[0][2] == res[1][2]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
