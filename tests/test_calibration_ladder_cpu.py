"""The maturity-ladder calibration driver and make_ladder_points without a GPU: the driver runs on an oracle-backed stand-in with
the ladder launchers' signatures (built the way tests/test_calibration_cpu.py builds its own: common.OracleSolver) and must walk
the same LM iterates as calibrate() fed the same prices point by point through the multi-maturity launchers."""
import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm

M1, M2 = 50, 25
START = (Cm.KAPPA, Cm.ETA, Cm.SIGMA, Cm.RHO, Cm.V_0)


class LadderOracleSolver(Cm.OracleSolver):
    """compute_jacobian_ladder / compute_base_prices_ladder by the ladder's definition: snapshot q is the single call with
    N = snap_steps[q] (one oracle solve per maturity: the stand-in has no sweep to take snapshots of).  Counts its calls."""

    def __init__(self):
        self.calls = []

    def compute_jacobian_ladder(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                num_strikes, grids, U_0, snap_steps, eps=1e-6, **kw):
        assert N == snap_steps[-1] and not kw
        self.calls.append("jac")
        parts = [self.compute_jacobian(S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, n, theta, delta_t,
                                       num_strikes, grids, U_0, eps=eps) for n in snap_steps]
        return np.stack([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)

    def compute_base_prices_ladder(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                   num_strikes, grids, ws, snap_steps, **kw):
        assert N == snap_steps[-1] and not kw
        self.calls.append("base")
        return np.stack([self.compute_base_prices(S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, n, theta,
                                                  delta_t, num_strikes, grids, ws) for n in snap_steps], axis=1)


def test_ladder_points_accepted():
    strikes = [95.0, 100.0, 105.0]
    pts = H.make_ladder_points(strikes, [0.25, 0.5, 1.0, 1.5], 0.05)
    assert len(pts) == 12 and [p.global_index for p in pts] == list(range(12))
    assert [p.time_steps for p in pts[::3]] == [5, 10, 20, 30] and all(p.delta_t == 0.05 for p in pts)
    assert pts[4] == H.CalibrationPoint(100.0, 0.5, 10, 0.05, 4)  # strike-fastest: m * len(strikes) + s
    # maturities formed as n * dt in floating point are whole numbers of steps to far within 1e-9
    dt = 1.0 / 30
    assert [p.time_steps for p in H.make_ladder_points([100.0], [k * dt for k in (3, 7, 30)], dt)] == [3, 7, 30]
    assert H.make_ladder_points([100.0], [0.05], 0.05)[0].time_steps == 1
    # the last maturity need not be anything special, and one maturity is a ladder too
    assert len(H.make_ladder_points(strikes, [0.35], 0.05)) == 3


@pytest.mark.parametrize("mats,dt", [([0.25, 0.52], 0.05), ([0.5 + 2e-9 * 0.05], 0.05), ([0.02], 0.05), ([0.0], 0.05), ([1.0], 0.3)])
def test_ladder_points_off_step_maturities_raise(mats, dt):
    with pytest.raises(ValueError, match="whole number"):
        H.make_ladder_points([100.0], mats, dt)


def test_ladder_points_just_inside_the_tolerance():
    assert H.make_ladder_points([100.0], [0.5 + 0.5e-9 * 0.05], 0.05)[0].time_steps == 10


@pytest.mark.parametrize("mats", [[0.5, 0.25], [0.5, 0.5], [0.25, 1.0, 0.75]])
def test_ladder_points_ordering(mats):
    with pytest.raises(ValueError, match="strictly increasing"):
        H.make_ladder_points([100.0], mats, 0.05)


def test_ladder_points_bad_step():
    for dt in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError):
            H.make_ladder_points([100.0], [0.5], dt)
    with pytest.raises(ValueError):
        H.make_ladder_points([100.0], [], 0.05)


@pytest.fixture(scope="module")
def surface():
    strikes, mats, dt = [92.0 + 4.0 * i for i in range(5)], [0.5, 0.75, 1.0, 1.5], 0.05
    pts = H.make_ladder_points(strikes, mats, dt)
    market = np.array([H.market.call_price(Cm.S_0, p.strike, Cm.R_D, 0.2, p.maturity) for p in pts])
    return strikes, mats, dt, pts, market


def test_driver_walks_the_iterates_of_the_point_by_point_driver(surface):
    strikes, mats, dt, pts, market = surface
    grids = H.GridViewsBatch.for_strikes(M1, M2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.call_payoff(strikes)
    lad = LadderOracleSolver()
    res = H.calibrate_european_maturity_ladder(lad, Cm.S_0, Cm.R_D, Cm.R_F, *START, M1, M2, Cm.THETA, strikes, mats, dt, grids,
                                               U0, market, max_iter=4)
    # the same prices point by point: one instance per (maturity, strike) with N_i = n_m on the shared dt
    ks = [p.strike for p in pts]
    grids_p = H.GridViewsBatch.for_strikes(M1, M2, Cm.S_0, Cm.V_0, ks)
    ref = H.calibrate_european_multi_maturity(Cm.OracleSolver(), Cm.S_0, Cm.R_D, Cm.R_F, *START, M1, M2, Cm.THETA, pts, grids_p,
                                              grids_p.call_payoff(ks), market, max_iter=4)
    assert res["iterations"] == ref["iterations"] >= 2 and res["converged"] == ref["converged"]
    for a, b in zip(res["history"], ref["history"]):
        assert a["params"] == b["params"] and a["trial"] == b["trial"] and a["error"] == b["error"] and a["lambda"] == b["lambda"]
        assert np.array_equal(a["delta"], b["delta"]) and a.get("trial_error") == b.get("trial_error")
    assert tuple(res[k] for k in ("kappa", "eta", "sigma", "rho", "v0")) == tuple(ref[k] for k in ("kappa", "eta", "sigma", "rho", "v0"))
    assert np.array_equal(res["model_prices"], ref["model_prices"])  # residual order m * len(strikes) + s
    # one launcher call per LM step, and the solve count is the sweeps actually run: one per strike and group
    assert lad.calls[0] == "jac" and lad.calls.count("jac") == res["iterations"]
    assert res["pde_solves"] == len(strikes) * 7 * res["iterations"] - len(strikes)


def test_driver_accepts_a_scheme_and_checks_its_inputs(surface):
    strikes, mats, dt, pts, market = surface
    grids = H.GridViewsBatch.for_strikes(M1, M2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.call_payoff(strikes)
    seen = {}

    class Recorder(LadderOracleSolver):
        def compute_jacobian_ladder(self, *a, **kw):
            seen.update(kw)
            kw.pop("scheme", None)
            return super().compute_jacobian_ladder(*a, **kw)

        def compute_base_prices_ladder(self, *a, **kw):
            kw.pop("scheme", None)
            return super().compute_base_prices_ladder(*a, **kw)

    H.calibrate_european_maturity_ladder(Recorder(), Cm.S_0, Cm.R_D, Cm.R_F, *START, M1, M2, 1.0 / 3.0, strikes, mats, dt, grids, U0,
                                         market, max_iter=1, scheme=2)
    assert seen["scheme"] == 2
    args = (Cm.S_0, Cm.R_D, Cm.R_F) + START + (M1, M2, Cm.THETA)
    with pytest.raises(ValueError, match="whole number"):
        H.calibrate_european_maturity_ladder(LadderOracleSolver(), *args, strikes, [0.5, 0.77], dt, grids, U0, market[:10])
    with pytest.raises(ValueError, match="one grid per strike"):
        H.calibrate_european_maturity_ladder(LadderOracleSolver(), *args, strikes[:3], mats, dt, grids, U0, market[:12])
    with pytest.raises(ValueError, match="market_prices"):
        H.calibrate_european_maturity_ladder(LadderOracleSolver(), *args, strikes, mats, dt, grids, U0, market[:7])


def test_existing_drivers_are_untouched(surface):
    """calibrate() without `launchers` builds its closures as before (the multi-maturity driver of the same points)."""
    strikes, mats, dt, pts, market = surface
    ks = [p.strike for p in pts]
    grids_p = H.GridViewsBatch.for_strikes(M1, M2, Cm.S_0, Cm.V_0, ks)
    U0 = grids_p.call_payoff(ks)
    a = H.calibrate(Cm.OracleSolver(), H.EU, Cm.S_0, None, Cm.R_D, Cm.R_F, *START, M1, M2, None, Cm.THETA, grids_p, U0, market,
                    calibration_points=pts, max_iter=1)
    b = H.calibrate(Cm.OracleSolver(), H.EU, Cm.S_0, None, Cm.R_D, Cm.R_F, *START, M1, M2, None, Cm.THETA, grids_p, U0, market,
                    calibration_points=pts, max_iter=1, launchers=None)
    assert a["history"][0]["error"] == b["history"][0]["error"]
