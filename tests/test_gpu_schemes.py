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
    b = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0)
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
