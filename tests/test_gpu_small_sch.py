"""hadi_small_sch_kernel on the device: Craig-Sneyd, Modified Craig-Sneyd and Hundsdorfer-Verwer sweeps of LDS-fitting grids as
one launch (tuning key "small_sch"), against the restatement tests/scheme_ref.py (1e-10 max|U_ref|, the bound of
test_gpu_schemes.py) and against the streaming kernels -- the same call with "small_sch" = 0 -- at their strip-vs-ring bound
(1e-11 max|U_ref|); the selection rule, the refusals, handle reuse, the Greeks, the calibration launchers' `scheme` and the
accuracy the schemes exist for.  Well-conditioned grids throughout (asserted)."""
import math

import numpy as np
import pytest

from oracle import oracle as O

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm
import scheme_ref as S

pytestmark = pytest.mark.gpu

TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
ALL = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
R_F = 0.007
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
NEW = "hadi_small_sch_kernel<"
# the emulator's shape list (tests/test_emu_small_sch.py says why each is there)
SHAPES = [(8, 4), (50, 25), (51, 7), (52, 8), (53, 31), (20, 30), (64, 32), (65, 16), (100, 20), (128, 32)]

_batches = {}


def _batch(m1, m2, n):
    """Grids and call payoffs of the first n well-conditioned strikes (built once per shape and size)."""
    if (m1, m2, n) not in _batches:
        strikes = Cm.well_conditioned_strikes(m1, n)
        grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
        Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
        _batches[(m1, m2, n)] = (grids, grids.call_payoff(strikes))
    return _batches[(m1, m2, n)]


def _run(sv, scheme, theta, m1, m2, N, grids, U0, small_sch, r_f=R_F, per=None, tuning=None):
    """One sweep with "small_sch" (and `tuning`) set for the call only -> (U_T, description)."""
    U = U0.copy()
    tuning = dict(tuning or {}, small_sch=small_sch)
    for k, v in tuning.items():
        sv.set_tuning(k, v)
    try:
        sv.DO_timestepping(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, *MODEL, grids, U, scheme=scheme, per_instance=per)
        return U, sv.describe_last_sweep()
    finally:
        for k in tuning:
            sv.set_tuning(k, -1)  # (every key used here goes back to its default with -1; "cs_strips": to 1)


def _ref_one(scheme, theta, m1, m2, grids, U0, k, N, dt, model=MODEL, r_f=R_F):
    p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, r_f, *model, O.EU)
    which = {H.SCHEME_CRAIG_SNEYD: S.CS, H.SCHEME_MCS: S.MCS, H.SCHEME_HV: S.HV}[scheme]
    return S.solve_one(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k], which)


def _cus(sv):
    return sv.device_info()["compute_units"]


# ---- 1. forced --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,theta,name", ALL, ids=[a[2] for a in ALL])
@pytest.mark.parametrize("m1,m2", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_forced_vs_restatement_and_streaming(solver, m1, m2, scheme, theta, name):
    n, N = 3, 4
    grids, U0 = _batch(m1, m2, n)
    U, d = _run(solver, scheme, theta, m1, m2, N, grids, U0, 1)
    Us, ds = _run(solver, scheme, theta, m1, m2, N, grids, U0, 0)
    assert NEW + "%d,%s>" % (1 if m1 <= 64 else 2, name) in d, d
    assert NEW not in ds and "row pass" in ds and ",%s>" % name in ds, ds
    for k in range(n):
        Uo = _ref_one(scheme, theta, m1, m2, grids, U0, k, N, Cm.T / N)
        mx = np.abs(Uo).max()
        e_ref, e_str = np.abs(U[k] - Uo).max() / mx, np.abs(U[k] - Us[k]).max() / mx
        print("%dx%d %s instance %d: vs restatement %.2e, vs streaming %.2e (of max|U|)" % (m1, m2, name, k, e_ref, e_str))
        assert e_ref <= 1e-10 and e_str <= 1e-11, (k, e_ref, e_str)


# ---- 2. automatic -----------------------------------------------------------------------------------------------------------
def test_automatic_above_one_instance_per_cu(solver):
    m1, m2, N = 50, 25, 4
    n = _cus(solver) + 1
    grids, U0 = _batch(m1, m2, n)
    U, d = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, -1)
    assert NEW + "1,MCS>" in d, d
    Us, ds = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, 0)
    assert NEW not in ds and "hadi_pass_a" in ds, ds
    mx = np.abs(Us).reshape(n, -1).max(axis=1)
    worst = (np.abs(U - Us).reshape(n, -1).max(axis=1) / mx).max()
    print("automatic, %d instances: worst vs streaming %.2e" % (n, worst))
    assert worst <= 1e-11
    for k in sorted(set([0, n - 1] + list(range(0, n, 32)))):
        Uo = _ref_one(H.SCHEME_MCS, TH_MCS, m1, m2, grids, U0, k, N, Cm.T / N)
        assert np.abs(U[k] - Uo).max() <= 1e-10 * np.abs(Uo).max(), k


def test_automatic_rule_keeps_the_streaming_kernels_elsewhere(solver):
    m1, m2, N = 50, 25, 2
    cus = _cus(solver)
    grids, U0 = _batch(m1, m2, cus + 1)
    sub = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), Cm.well_conditioned_strikes(m1, cus))
    _, d = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, sub, U0[:cus].copy(), -1)  # one instance per CU: streaming
    assert NEW not in d and "hadi_pass_a" in d, d
    for tuning in ({"strip": 1}, {"cs_strips": 0}):  # pinned streaming geometry
        _, d = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, -1, tuning=tuning)
        assert NEW not in d and "hadi_pass_a" in d, (tuning, d)
    g129, U129 = _batch(129, 32, cus + 1)  # not admitted
    _, d = _run(solver, H.SCHEME_MCS, TH_MCS, 129, 32, N, g129, U129, -1)
    assert NEW not in d and "hadi_pass_a" in d, d
    _, d = _run(solver, H.SCHEME_MCS, TH_MCS, 129, 32, N, g129, U129, 1)  # ... and forcing does not admit it
    assert NEW not in d, d
    g100, U100 = _batch(100, 20, cus + 1)  # admitted, but a CU's LDS holds two instances, not three: measured slower, stays streaming
    _, d = _run(solver, H.SCHEME_MCS, TH_MCS, 100, 20, N, g100, U100, -1)
    assert NEW not in d and "hadi_pass_a" in d, d
    _, d = _run(solver, H.SCHEME_MCS, TH_MCS, 100, 20, N, g100, U100, 1)
    assert NEW + "2,MCS>" in d, d
    _, d = _run(solver, H.SCHEME_DOUGLAS, 0.5, m1, m2, N, grids, U0, -1)  # Douglas: as before
    assert "hadi_small_seq" in d, d


# ---- 3. mixed maturities ----------------------------------------------------------------------------------------------------
def test_mixed_maturities_and_per_instance_parameters(solver):
    m1, m2 = 50, 25
    n = _cus(solver) + 1
    grids, U0 = _batch(m1, m2, n)
    models = [(-0.9, 0.3, 1.5, 0.04), (-0.5, 0.5, 2.0, 0.09), (0.0, 0.2, 0.5, 0.02), (0.3, 0.4, 3.0, 0.06)]
    Ns = [(6, 1, 4, 2)[k % 4] for k in range(n)]
    Ts = [(0.5, 1.0, 0.8, 0.25)[k % 4] for k in range(n)]
    per = dict(rho_i=[models[k % 4][0] for k in range(n)], sigma_i=[models[k % 4][1] for k in range(n)],
               kappa_i=[models[k % 4][2] for k in range(n)], eta_i=[models[k % 4][3] for k in range(n)],
               N_i=Ns, delta_t_i=[t / s for t, s in zip(Ts, Ns)])
    for scheme, theta, name in ALL[1:]:
        U, d = _run(solver, scheme, theta, m1, m2, 1, grids, U0, -1, per=per)
        assert NEW in d and ",%s>" % name in d, d
        Us, ds = _run(solver, scheme, theta, m1, m2, 1, grids, U0, 0, per=per)
        assert NEW not in ds, ds
        mx = np.abs(Us).reshape(n, -1).max(axis=1)
        assert (np.abs(U - Us).reshape(n, -1).max(axis=1) / mx).max() <= 1e-11
        for k in range(8):
            Uo = _ref_one(scheme, theta, m1, m2, grids, U0, k, Ns[k], Ts[k] / Ns[k], models[k % 4])
            assert np.abs(U[k] - Uo).max() <= 1e-10 * np.abs(Uo).max(), (name, k)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,theta,name", ALL[1:], ids=["MCS", "HV"])
def test_refusals_unchanged_when_forced(solver, scheme, theta, name):
    m1, m2, N = 50, 25, 4
    grids, U0 = _batch(m1, m2, 1)
    strike = Cm.well_conditioned_strikes(m1, 1)
    cases = [dict(variant=H.AM, U_0=U0), dict(variant=H.DIV, dividends=H.Dividends(*Cm.DIVS)),
             dict(option_type=H.PUT, strikes=strike), dict(state_precision=H.STATE_FP32)]
    solver.set_tuning("small_sch", 1)
    try:
        for kw in cases + [dict(theta=0.0)]:
            th = kw.pop("theta", theta)
            with pytest.raises(H.HadiError) as e:
                solver.DO_timestepping(m1, m2, N, Cm.T / N, th, Cm.R_D, R_F, *MODEL, grids, U0.copy(), scheme=scheme, **kw)
            assert e.value.status == 2, kw
    finally:
        solver.set_tuning("small_sch", -1)


# ---- 5. handle reuse --------------------------------------------------------------------------------------------------------
def test_handle_reuse_across_paths(solver):
    grids, U0 = _batch(50, 25, 3)
    a, d = _run(solver, H.SCHEME_MCS, TH_MCS, 50, 25, 4, grids, U0, 1)
    assert NEW in d, d
    gb, Ub = _batch(130, 70, 2)
    _, db = _run(solver, H.SCHEME_MCS, TH_MCS, 130, 70, 3, gb, Ub, 1)  # not admitted: the streaming kernels and their HBM arrays
    assert NEW not in db and "hadi_pass_a" in db, db
    b, d = _run(solver, H.SCHEME_MCS, TH_MCS, 50, 25, 4, grids, U0, 1)
    assert NEW in d and np.array_equal(a, b)
    with H.HestonADI(0) as fresh:
        c, d = _run(fresh, H.SCHEME_MCS, TH_MCS, 50, 25, 4, grids, U0, 1)
        assert NEW in d and np.array_equal(a, c)


# ---- 6. Greeks --------------------------------------------------------------------------------------------------------------
def test_greeks_read_the_state_the_kernel_leaves(solver):
    m1, m2, N = 50, 25, 4
    grids, U0 = _batch(m1, m2, 3)
    V0 = Cm.v0_for(m2)
    solver.set_tuning("small_sch", 1)
    try:
        out, lad = solver.compute_greeks(m1, m2, N, Cm.T / N, TH_MCS, Cm.R_D, R_F, *MODEL, grids, U0.copy(), Cm.S_0, V0,
                                         scheme=H.SCHEME_MCS, ladder=True)
        d = solver.describe_last_sweep()
    finally:
        solver.set_tuning("small_sch", -1)
    assert NEW + "1,MCS>" in d, d
    U, _ = _run(solver, H.SCHEME_MCS, TH_MCS, m1, m2, N, grids, U0, 1)
    for k in range(3):
        i0, j0 = O.find_s_index(grids.Vec_s[k], Cm.S_0), O.find_v_index(grids.Vec_v[k], V0)
        row = U[k].reshape(m2 + 1, m1 + 1)[j0]
        assert out[k, H.G_PRICE] == row[i0]
        assert np.array_equal(lad[k, :, H.G_PRICE], row)


# ---- 7. calibration interface -----------------------------------------------------------------------------------------------
def test_jacobian_and_base_prices_take_the_scheme(solver):
    m1, m2, N, n = 50, 25, 20, 60
    strikes = Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(strikes)
    args = (Cm.S_0, Cm.V_0, Cm.T, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, m1, m2, (m1 + 1) * (m2 + 1), N, TH_MCS, Cm.T / N,
            n, grids, U0)
    J, base = solver.compute_jacobian(*args, eps=1e-6, scheme=H.SCHEME_MCS)
    d = solver.describe_last_sweep()
    if _cus(solver) < 6 * n:
        assert NEW + "1,MCS>" in d, d
    solver.set_tuning("small_sch", 0)
    try:
        Js, bases = solver.compute_jacobian(*args, eps=1e-6, scheme=H.SCHEME_MCS)
        ds = solver.describe_last_sweep()
    finally:
        solver.set_tuning("small_sch", -1)
    assert NEW not in ds and ",MCS>" in ds, ds
    vv, dv = O.rebuild_variance(m2, Cm.V_0)
    iv = O.find_v_index(vv, Cm.V_0)
    p = O.make_params(m1, m2, N, Cm.T / N, TH_MCS, Cm.R_D, R_F, *MODEL, O.EU)
    ref = np.array([S.solve_one(p, grids.Vec_s[k], vv, grids.Delta_s[k], dv, U0[k], S.MCS)[iv * (m1 + 1) + O.find_s_index(grids.Vec_s[k], Cm.S_0)]
                    for k in range(n)])
    print("base vs restatement %.2e, J vs streaming %.2e" % (np.abs(base - ref).max(), np.abs(J - Js).max()))
    assert np.abs(base - ref).max() <= 1e-9
    assert np.abs(J - Js).max() <= 2e-4
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1))
    ws.U[...] = U0
    bp = solver.compute_base_prices(*args[:-1], ws, scheme=H.SCHEME_MCS)
    assert np.abs(bp - base).max() <= 1e-12
    # Douglas at this theta prices differently: the keyword reached the library
    ws.U[...] = U0
    assert np.abs(solver.compute_base_prices(*args[:-1], ws) - base).max() > 1e-6


# ---- 8. accuracy ------------------------------------------------------------------------------------------------------------
def test_accuracy_against_douglas_at_twenty_steps(solver):
    """Time error at N = 20 (scheme_ref.time_error) against HV at N = 4000, everything but Douglas on the new kernel: MCS at
    least 20x and HV at least 8x below Douglas, the ratios test_gpu_schemes.py holds for the streaming kernels."""
    m1, m2 = 50, 25
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, [100.0])
    U0 = grids.call_payoff([100.0])

    def run(scheme, theta, N):
        U, d = _run(solver, scheme, theta, m1, m2, N, grids, U0, 1, r_f=Cm.R_F)
        assert (NEW in d) == (scheme != 0), d
        return U[0]

    ref = run(H.SCHEME_HV, TH_HV, 4000)
    err = lambda U: S.time_error(U, ref, grids.Vec_s[0], grids.Vec_v[0], m1, m2)
    e_do, e_mcs, e_hv = err(run(0, 0.5, 20)), err(run(H.SCHEME_MCS, TH_MCS, 20)), err(run(H.SCHEME_HV, TH_HV, 20))
    print("time error at N = 20: Douglas %.3e, MCS %.3e, HV %.3e" % (e_do, e_mcs, e_hv))
    assert e_mcs <= e_do / 20 and e_hv <= e_do / 8, (e_do, e_mcs, e_hv)
