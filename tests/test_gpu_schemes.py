"""Modified Craig-Sneyd and Hundsdorfer-Verwer on the device (HADI_SCHEME_MCS / HADI_SCHEME_HV) against the test-side
restatement tests/scheme_ref.py (oracle operators and line solves), against the shared-ring kernels, against libhadi_strict.so
(every counted wait a full drain), and the accuracy that is the reason for them."""
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm
import scheme_ref as S

pytestmark = pytest.mark.gpu

TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
R_F = 0.007


@pytest.fixture(scope="module")
def strict_solver():
    """libhadi_strict.so: the same sources with every counted `s_waitcnt vmcnt(n)` replaced by a full drain."""
    import __graft_entry__ as G
    s = H.HestonADI(0, lib_path=G.build_libhadi_strict())
    yield s
    s.close()


def _batch(m1, m2, strikes):
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    return grids, grids.call_payoff(strikes)


def _run(sv, scheme, theta, m1, m2, N, grids, U0, r_f=R_F):
    U = U0.copy()
    sv.DO_timestepping(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U, scheme=scheme)
    return U


def _ref(scheme, theta, m1, m2, N, grids, U0, r_f=R_F):
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=r_f)
    return S.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, scheme, theta)


def _rel(U, Uo):
    return np.abs(U - Uo).max() / np.abs(Uo).max()


@pytest.mark.parametrize("scheme,theta,name", SCHEMES)
@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 20, 4), (128, 64, 8, 2), (512, 256, 6, 2), (700, 300, 3, 1)])
def test_full_field_vs_restatement(solver, scheme, theta, name, m1, m2, N, n):
    """Craig-Sneyd's shape set: the first two are batches the Douglas path would run on the LDS-resident small kernels, the
    third is a team-kernel shape -- a scheme that fell into either would silently run Douglas."""
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    U = _run(solver, scheme, theta, m1, m2, N, grids, U0)
    d = solver.describe_last_sweep()
    assert ",%s>" % name in d, d
    assert _rel(U, _ref(scheme, theta, m1, m2, N, grids, U0)) <= 1e-10


@pytest.mark.parametrize("scheme,theta,name", SCHEMES)
@pytest.mark.parametrize("m1,m2,N,n", [(100, 50, 5, 3), (256, 128, 5, 2), (400, 131, 5, 2), (512, 256, 6, 2), (600, 40, 5, 2),
                                       (1024, 100, 4, 1)])
def test_on_strips_vs_restatement_ring_and_full_drains(solver, strict_solver, scheme, theta, name, m1, m2, N, n):
    """Predictor and corrector on the barrier-free strips (2, 4, 8 nodes per lane; paired strips above 512 s-intervals):
    against the restatement, against the shared ring (`cs_strips` = 0) to round-off, and bit for bit against the build whose
    waits drain everything."""
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    solver.set_tuning("strip", 1)
    try:
        U = _run(solver, scheme, theta, m1, m2, N, grids, U0)
        d = solver.describe_last_sweep()
        solver.set_tuning("cs_strips", 0)
        Ur = _run(solver, scheme, theta, m1, m2, N, grids, U0)
        dr = solver.describe_last_sweep()
    finally:
        solver.set_tuning("cs_strips", 1)
        solver.set_tuning("strip", -1)
    B = 2 if m1 <= 128 else 4 if m1 <= 256 else 8
    assert ("hadi_pass_a_strip_sch<8,EU,double,2,%s>" % name if m1 > 512 else "hadi_pass_a_strip_sch<%d,EU,double,1,%s>" % (B, name)) in d, d
    assert "strip" not in dr and "hadi_pass_a_sch<" in dr and ",%s>" % name in dr, dr
    Uo = _ref(scheme, theta, m1, m2, N, grids, U0)
    assert _rel(U, Uo) <= 1e-10
    assert np.abs(U - Ur).max() <= 1e-11 * np.abs(Uo).max()
    strict_solver.set_tuning("strip", 1)
    try:
        Us = _run(strict_solver, scheme, theta, m1, m2, N, grids, U0)
        assert strict_solver.describe_last_sweep() == d
    finally:
        strict_solver.set_tuning("strip", -1)
    assert np.array_equal(U, Us)


@pytest.mark.parametrize("m1,m2,N,n", [(50, 25, 20, 4), (300, 80, 6, 2), (700, 300, 3, 1)])
def test_mcs_at_one_half_is_craig_sneyd(solver, m1, m2, N, n):
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    U = _run(solver, H.SCHEME_MCS, 0.5, m1, m2, N, grids, U0)
    Uc = _run(solver, H.SCHEME_CRAIG_SNEYD, 0.5, m1, m2, N, grids, U0)
    assert _rel(U, Uc) <= 1e-12


def test_mcs_on_strips_under_load_equals_full_drains(solver, strict_solver):
    """256 instances of 512x256 (the plan picks the strips by itself) over 40 steps, every CU streaming: bit for bit against
    the build whose counted waits drain everything."""
    m1, m2, N, n = 512, 256, 40, 256
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    U = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, r_f=0.01)
    d = solver.describe_last_sweep()
    assert "hadi_pass_a_strip_sch<8,EU,double,1,MCS>" in d, d
    Us = _run(strict_solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, r_f=0.01)
    assert strict_solver.describe_last_sweep() == d
    assert np.array_equal(U, Us)
    assert np.isfinite(U).all() and np.abs(U).max() < 1e4


def test_graph_replay_does_not_cross_schemes(solver):
    """Small batches replay a captured time loop; the graph key holds the scheme.  The same MCS call twice is bit-identical,
    and MCS, CS, HV in a row on one handle each equal a fresh handle's result."""
    m1, m2, N, n = 50, 25, 20, 4
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    a = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0)
    g0 = Cm.graph_counts(solver)
    b = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0)
    dg = Cm.graph_delta(g0, Cm.graph_counts(solver))
    assert dg["replays"] == 1 and dg["captures"] == 0, dg  # the second call really replayed
    assert np.array_equal(a, b)
    seq = [(H.SCHEME_MCS, TH_MCS), (H.SCHEME_CRAIG_SNEYD, TH_MCS), (H.SCHEME_HV, TH_MCS)]
    got = [_run(solver, sc, th, m1, m2, N, grids, U0) for sc, th in seq]
    for (sc, th), g in zip(seq, got):
        with H.HestonADI(0) as fresh:
            assert np.array_equal(g, _run(fresh, sc, th, m1, m2, N, grids, U0)), sc
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


def test_accuracy_against_douglas_at_twenty_steps(solver):
    """The reason for the schemes: time error at N = 20 (max over s in [50, 150], v <= 1, K = 100) against HV at N = 4000 on
    the same space grid -- MCS at least 20x and HV at least 8x below Douglas (measured: 45x and 13x at least); the two fine
    solutions agree."""
    for m1, m2 in ((50, 25), (60, 30), (100, 50)):
        grids, U0 = _batch(m1, m2, [100.0])

        def run(scheme, theta, N):
            return _run(solver, scheme, theta, m1, m2, N, grids, U0, r_f=Cm.R_F)[0]

        ref = run(H.SCHEME_HV, TH_HV, 4000)
        ref_mcs = run(H.SCHEME_MCS, TH_MCS, 4000)
        err = lambda U: S.time_error(U, ref, grids.Vec_s[0], grids.Vec_v[0], m1, m2)
        e_do, e_mcs, e_hv = err(run(0, 0.5, 20)), err(run(H.SCHEME_MCS, TH_MCS, 20)), err(run(H.SCHEME_HV, TH_HV, 20))
        assert e_mcs <= e_do / 20 and e_hv <= e_do / 8, (m1, m2, e_do, e_mcs, e_hv)
        assert np.abs(ref - ref_mcs).max() <= 2e-5


@pytest.mark.parametrize("scheme,theta,name", SCHEMES)
def test_refusals(solver, scheme, theta, name):
    m1, m2, N = 50, 25, 4
    grids, U0 = _batch(m1, m2, [100.0])
    cases = [dict(variant=H.AM, U_0=U0), dict(variant=H.DIV, dividends=H.Dividends(*Cm.DIVS)),
             dict(option_type=H.PUT, strikes=[100.0]), dict(state_precision=H.STATE_FP32)]
    for kw in cases:
        with pytest.raises(H.HadiError) as e:
            solver.DO_timestepping(m1, m2, N, Cm.T / N, theta, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U0.copy(),
                                   scheme=scheme, **kw)
        assert e.value.status == 2, kw
    with pytest.raises(H.HadiError) as e:  # theta = 0
        solver.DO_timestepping(m1, m2, N, Cm.T / N, 0.0, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U0.copy(),
                               scheme=scheme)
    assert e.value.status == 2
    g2, V0 = _batch(1100, 30, [100.0])  # m1 > 1024: the sequential passes run Douglas only
    with pytest.raises(H.HadiError) as e:
        solver.DO_timestepping(1100, 30, 2, Cm.T / 2, theta, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, g2, V0.copy(),
                               scheme=scheme)
    assert e.value.status == 2


# ---- per-instance inputs, mixed strip / ring passes, theta and r_f, shape edges, HV under load ---------------------------
ALL = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS")] + SCHEMES
PER4 = dict(rho_i=[-0.9, -0.5, 0.0, 0.3], sigma_i=[0.3, 0.5, 0.2, 0.4], kappa_i=[1.5, 2.0, 0.5, 3.0], eta_i=[0.04, 0.09, 0.02, 0.06])
TS4, NS4 = [0.5, 1.0, 0.8, 0.25], [5, 8, 3, 2]


def _ref_one(scheme, theta, m1, m2, grids, U0, k, N, dt, model, r_f):
    """Instance k against its own reference solve: the oracle for Craig-Sneyd, the restatement for MCS / HV."""
    from oracle import oracle as O
    p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, r_f, *model, O.EU, scheme=1 if scheme == H.SCHEME_CRAIG_SNEYD else 0)
    g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
    if scheme == H.SCHEME_CRAIG_SNEYD:
        return O.solve(p, *g, U0[k])[0]
    return S.solve_one(p, *g, U0[k], S.MCS if scheme == H.SCHEME_MCS else S.HV)


def _check_ref(scheme, theta, m1, m2, grids, U0, U, r_f, N, per=None):
    for k in range(U.shape[0]):
        if per:
            model = (per["rho_i"][k], per["sigma_i"][k], per["kappa_i"][k], per["eta_i"][k])
            Nk, dtk = per["N_i"][k], per["delta_t_i"][k]
        else:
            model, Nk, dtk = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA), N, Cm.T / N
        Uo = _ref_one(scheme, theta, m1, m2, grids, U0, k, Nk, dtk, model, r_f)
        assert _rel(U[k], Uo) <= 1e-10, (k, _rel(U[k], Uo))


def _tuned(sv, tuning):
    for k, v in tuning.items():
        sv.set_tuning(k, v)


def _untune(sv, tuning):
    defaults = {"strip": -1, "cs_strips": 1, "pair_strips": -1, "col_prefetch": 0, "tile_interleave": 0, "graph": 1, "team_launch": -1}
    for k in tuning:
        sv.set_tuning(k, defaults[k])


@pytest.mark.parametrize("scheme,theta,name", ALL)
@pytest.mark.parametrize("path,m1,m2,tuning", [
    ("graph", 50, 25, {}), ("ring", 200, 60, {"strip": 1, "cs_strips": 0}), ("strips2", 100, 50, {"strip": 1}),
    ("strips4", 200, 60, {"strip": 1}), ("strips8", 300, 80, {"strip": 1}), ("paired600", 600, 40, {"strip": 1}),
    ("paired1024", 1024, 100, {"strip": 1})])
def test_per_instance_parameters_and_maturities(solver, scheme, theta, name, path, m1, m2, tuning):
    """rho_i / sigma_i / kappa_i / eta_i and N_i / delta_t_i: every kernel of a scheme takes dt, theta dt, e_n / e_{n-1} and the
    scheme's constants from its own instance and stops at its own N (the strips drain their row fetches first)."""
    strikes = [90.0, 100.0, 110.0, 95.0]
    per = dict(PER4, N_i=NS4, delta_t_i=[t / n for t, n in zip(TS4, NS4)])
    grids, U0 = _batch(m1, m2, strikes)
    _tuned(solver, tuning)
    try:
        for call in range(2 if path == "graph" else 1):  # (graph: the second call replays the captured time loop)
            U = U0.copy()
            g0 = Cm.graph_counts(solver)
            solver.DO_timestepping(m1, m2, 1, 1.0, theta, Cm.R_D, R_F, 0.0, 0.1, 1.0, 0.04, grids, U, scheme=scheme, per_instance=per)
            if call == 1:
                dg = Cm.graph_delta(g0, Cm.graph_counts(solver))
                assert dg["replays"] == 1 and dg["captures"] == 0, dg
        d = solver.describe_last_sweep()
    finally:
        _untune(solver, tuning)
    B = 2 if m1 <= 128 else 4 if m1 <= 256 else 8
    strip_k = "hadi_pass_a_strip" if scheme == H.SCHEME_CRAIG_SNEYD else "hadi_pass_a_strip_sch"
    ring_k = "hadi_pass_a<" if scheme == H.SCHEME_CRAIG_SNEYD else "hadi_pass_a_sch<"
    if path in ("graph", "ring"):
        assert "strip" not in d and ring_k in d and ",%s>" % name in d, d
    elif m1 > 512:
        assert "%s<8,EU,double,2,%s>" % (strip_k, name) in d, d
    else:
        assert "%s<%d,EU,double,1,%s>" % (strip_k, B, name) in d, d
    _check_ref(scheme, theta, m1, m2, grids, U0, U, R_F, None, per)


@pytest.mark.parametrize("scheme,theta,name", ALL)
@pytest.mark.parametrize("m1,m2,N,n", [(100, 50, 4, 2), (200, 60, 4, 2), (300, 80, 4, 2)])
def test_predictor_or_corrector_alone_on_strips(solver, scheme, theta, name, m1, m2, N, n):
    """`cs_strips` = 2 (predictor on strips, corrector on the shared ring) and 3 (the other way round): the strip and ring
    kernels hand each other the R1 / C2 carry-over rows.  Both agree to round-off with all-strips (1) and all-ring (0)."""
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    out = {}
    solver.set_tuning("strip", 1)
    try:
        for cs in (0, 1, 2, 3):
            solver.set_tuning("cs_strips", cs)
            out[cs] = (_run(solver, scheme, theta, m1, m2, N, grids, U0), solver.describe_last_sweep())
    finally:
        solver.set_tuning("cs_strips", 1)
        solver.set_tuning("strip", -1)
    assert "strip" not in out[0][1] and all("strip" in out[cs][1] for cs in (1, 2, 3)), out
    Uo = _ref(scheme, theta, m1, m2, N, grids, U0)
    for cs in (0, 1, 2, 3):
        assert _rel(out[cs][0], Uo) <= 1e-10, cs
    for cs in (2, 3):
        assert np.abs(out[cs][0] - out[1][0]).max() <= 1e-11 * np.abs(Uo).max(), cs
        assert np.abs(out[cs][0] - out[0][0]).max() <= 1e-11 * np.abs(Uo).max(), cs


THETAS = [(H.SCHEME_MCS, 0.75, "MCS"), (H.SCHEME_MCS, 1.0, "MCS"), (H.SCHEME_HV, 0.5, "HV"), (H.SCHEME_HV, 1.0, "HV"),
          (H.SCHEME_CRAIG_SNEYD, 0.0, "CS"), (H.SCHEME_CRAIG_SNEYD, 1.0, "CS")]


@pytest.mark.parametrize("scheme,theta,name", THETAS)
@pytest.mark.parametrize("r_f", [0.0, Cm.R_D, 0.06], ids=["rf0", "rf_eq_rd", "rf_gt_rd"])
def test_theta_and_rates(solver, scheme, theta, name, r_f):
    """MCS above 1/2 and at 1, HV at 1/2 and 1 (the strips' kap = 0), CS at 0 and 1; r_f = r_d (the library keeps the strips
    off: forced strips must fall back to the shared ring) and r_f > r_d.  Forced strips at 8 nodes per lane.  (Explicit CS takes
    one step: more steps of this size grow without bound, and the round-off with them.)"""
    m1, m2, N = 300, 34, 1 if theta == 0.0 else 4
    grids, U0 = _batch(m1, m2, [100.0, 93.0])
    solver.set_tuning("strip", 1)
    try:
        U = _run(solver, scheme, theta, m1, m2, N, grids, U0, r_f=r_f)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("strip", -1)
    if r_f == Cm.R_D or theta == 0.0:
        assert "strip" not in d and ",%s>" % name in d, d
    else:
        assert "<8,EU,double,1,%s>" % name in d and "strip" in d, d
    assert _rel(U, _ref(scheme, theta, m1, m2, N, grids, U0, r_f=r_f)) <= 1e-10


@pytest.mark.parametrize("m1", [128, 129, 256, 257, 512, 513])
@pytest.mark.parametrize("m2", [3, 263, 264])
def test_plan_boundaries(solver, m1, m2):
    """The plan's boundaries in m1 (nodes per lane 2 | 4 | 8 | paired) against m2 = 3 (four v-rows), 263 (8 chunks) and 264
    (9 chunks: the 1024-thread column pass); the three schemes in turn, N = 2, on strips where the plan allows them."""
    scheme, theta, name = ALL[(m1 + m2) % 3]
    grids, U0 = _batch(m1, m2, [100.0])
    solver.set_tuning("strip", 1)
    try:
        U = _run(solver, scheme, theta, m1, m2, 2, grids, U0, r_f=0.01)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("strip", -1)
    assert ",%s>" % name in d, d
    assert _rel(U, _ref(scheme, theta, m1, m2, 2, grids, U0, r_f=0.01)) <= 1e-10


@pytest.mark.parametrize("scheme,theta,name", SCHEMES)
def test_largest_admitted_shape(solver, scheme, theta, name):
    m1, m2 = 1024, 527
    grids, U0 = _batch(m1, m2, [100.0])
    U = _run(solver, scheme, theta, m1, m2, 2, grids, U0)
    assert ",%s>" % name in solver.describe_last_sweep()
    assert _rel(U, _ref(scheme, theta, m1, m2, 2, grids, U0)) <= 1e-10


@pytest.mark.parametrize("scheme,theta,name", ALL)
@pytest.mark.parametrize("m1,m2", [(300, 264), (200, 527)])
def test_prefetching_column_pass_with_interleaved_tiles(solver, scheme, theta, name, m1, m2):
    """9 .. 16 chunks with `col_prefetch` (hadi_pass_b2) and `tile_interleave`: the scheme's column passes read V and U."""
    grids, U0 = _batch(m1, m2, [100.0, 92.0])
    tuning = {"col_prefetch": 1, "tile_interleave": 1, "strip": 1}
    _tuned(solver, tuning)
    try:
        U = _run(solver, scheme, theta, m1, m2, 2, grids, U0)
        d = solver.describe_last_sweep()
    finally:
        _untune(solver, tuning)
    assert "hadi_pass_b2<16" in d and ",%s>" % name in d, d
    assert _rel(U, _ref(scheme, theta, m1, m2, 2, grids, U0)) <= 1e-10


@pytest.mark.parametrize("scheme,theta,name", ALL)
def test_pair_strip_plans_send_the_scheme_to_the_ring(solver, scheme, theta, name):
    """Forced `pair_strips` on 256x128 (hadi_pass_a_pairs is a Douglas kernel): the scheme's passes run on the shared ring."""
    m1, m2, N = 256, 128, 3
    grids, U0 = _batch(m1, m2, Cm.strikes_for(2))
    tuning = {"strip": 1, "pair_strips": 1, "team_launch": 0}
    _tuned(solver, tuning)
    try:
        U = _run(solver, scheme, theta, m1, m2, N, grids, U0)
        d = solver.describe_last_sweep()
        U_do = U0.copy()
        solver.DO_timestepping(m1, m2, N, Cm.T / N, 0.5, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U_do)
        d_do = solver.describe_last_sweep()
    finally:
        _untune(solver, tuning)
    assert "hadi_pass_a_pairs" in d_do, d_do  # (the plan does pick the pairs)
    assert "strip" not in d and "pairs" not in d and ",%s>" % name in d, d
    assert _rel(U, _ref(scheme, theta, m1, m2, N, grids, U0)) <= 1e-10


@pytest.mark.parametrize("scheme,theta,name", ALL)
def test_refusals_beyond_the_streaming_shapes(solver, scheme, theta, name):
    for m1, m2 in ((100, 528), (1025, 30)):
        grids, U0 = _batch(m1, m2, [100.0])
        with pytest.raises(H.HadiError) as e:
            _run(solver, scheme, theta, m1, m2, 2, grids, U0)
        assert e.value.status == 2, (m1, m2)


@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed_N"])
def test_hv_on_strips_under_load_equals_full_drains(solver, strict_solver, mixed):
    """256 instances of 512x256 over 40 steps on strips, bit for bit against the build whose counted waits drain everything;
    mixed_N: N_i of 40, 13, 27 and 1 steps side by side, so blocks that leave at once (after draining their row fetches) run
    beside blocks that stream."""
    m1, m2, N, n = 512, 256, 40, 256
    grids, U0 = _batch(m1, m2, Cm.strikes_for(n))
    per = None
    if mixed:
        Ns = [(40, 13, 27, 1)[k % 4] for k in range(n)]
        per = dict(N_i=Ns, delta_t_i=[Cm.T / x for x in Ns])

    def run(sv):
        U = U0.copy()
        sv.DO_timestepping(m1, m2, N, Cm.T / N, TH_HV, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                           scheme=H.SCHEME_HV, per_instance=per)
        return U, sv.describe_last_sweep()

    U, d = run(solver)
    assert "hadi_pass_a_strip_sch<8,EU,double,1,HV>" in d, d
    Us, ds = run(strict_solver)
    assert ds == d
    assert np.array_equal(U, Us)
    assert np.isfinite(U).all() and np.abs(U).max() < 1e4
    if mixed:  # two of the short instances against the restatement
        for k in (1, 3):
            Uo = _ref_one(H.SCHEME_HV, TH_HV, m1, m2, grids, U0, k, Ns[k], Cm.T / Ns[k], (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA), 0.01)
            assert _rel(U[k], Uo) <= 1e-10, k
