"""The calibration drivers hand `scheme` to every Jacobian and trial-price call (CPU only).  The stand-in below has the European
launchers' signatures WITH the keyword and prices with the restatement tests/scheme_ref.py; common.OracleSolver, which takes
no `scheme`, must keep working with the drivers when the argument is left out."""
import numpy as np
import pytest

from oracle import oracle as O

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import calibration as Cal

import common as Cm
import scheme_ref as S

M1, M2, N = 20, 10, 4
STRIKES = [95.0, 100.0, 105.0]
TRUE = dict(kappa=1.5, eta=0.04, sigma=0.3, rho=-0.9, v0=0.04)
START = dict(kappa=1.2, eta=0.05, sigma=0.35, rho=-0.7, V_0=0.05)


class SchemeOracleSolver(Cm.OracleSolver):
    """compute_jacobian / compute_base_prices (and the multi-maturity pair) with the `scheme` keyword of HestonADI's: the price
    of instance k is the restatement's field at (S_0, V_0) on the v-grid rebuilt around V_0, the Jacobian its forward
    differences in (kappa, eta, sigma, rho, v0).  Every call's scheme is recorded."""

    def __init__(self):
        self.calls = []

    def _prices(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, steps, grids, U, scheme):
        vv, dv = O.rebuild_variance(m2, V_0)
        iv = O.find_v_index(vv, V_0)
        out = np.empty(len(steps))
        for k, (Nk, dtk) in enumerate(steps):
            p = O.make_params(m1, m2, Nk, dtk, theta, r_d, r_f, rho, sigma, kappa, eta, O.EU)
            Uk = S.solve_one(p, grids.Vec_s[k], vv, grids.Delta_s[k], dv, np.asarray(U)[k], scheme)
            out[k] = Uk[iv * (m1 + 1) + O.find_s_index(grids.Vec_s[k], S_0)]
        return out

    def _jac_fd(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, steps, grids, U_0, eps, scheme):
        base = self._prices(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, steps, grids, U_0, scheme)
        J = np.empty((len(steps), 5))
        for col, bump in enumerate(("kappa", "eta", "sigma", "rho", "V_0")):
            a = dict(kappa=kappa, eta=eta, sigma=sigma, rho=rho, V_0=V_0)
            a[bump] += eps
            J[:, col] = (self._prices(S_0, a["V_0"], r_d, r_f, a["rho"], a["sigma"], a["kappa"], a["eta"], m1, m2, theta, steps,
                                      grids, U_0, scheme) - base) / eps
        return J, base

    def compute_jacobian(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                         num_strikes, grids, U_0, eps=1e-6, scheme=0):
        self.calls.append(("jac", scheme))
        return self._jac_fd(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, [(N, delta_t)] * num_strikes, grids, U_0, eps, scheme)

    def compute_base_prices(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                            num_strikes, grids, ws, scheme=0):
        self.calls.append(("base", scheme))
        return self._prices(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, [(N, delta_t)] * num_strikes, grids, ws.U, scheme)

    def compute_jacobian_multi_maturity(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, theta, points, n,
                                        grids, U_0, eps=1e-6, scheme=0):
        self.calls.append(("jac_mm", scheme))
        return self._jac_fd(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, [(p.time_steps, p.delta_t) for p in points],
                            grids, U_0, eps, scheme)

    def compute_base_prices_multi_maturity(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, theta, points,
                                           n, grids, ws, scheme=0):
        self.calls.append(("base_mm", scheme))
        return self._prices(S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, theta, [(p.time_steps, p.delta_t) for p in points],
                            grids, ws.U, scheme)


def _setup(strikes=STRIKES):
    grids = H.GridViewsBatch.for_strikes(M1, M2, Cm.S_0, START["V_0"], strikes)
    return grids, grids.call_payoff(strikes)


def test_european_driver_hands_the_scheme_to_every_launcher_call():
    grids, U_0 = _setup()
    sv = SchemeOracleSolver()
    theta = 1.0 / 3.0
    steps = [(N, Cm.T / N)] * len(STRIKES)
    market = sv._prices(Cm.S_0, TRUE["v0"], Cm.R_D, Cm.R_F, TRUE["rho"], TRUE["sigma"], TRUE["kappa"], TRUE["eta"], M1, M2, theta,
                        steps, grids, U_0, S.MCS)
    res = Cal.calibrate_european(sv, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, START["kappa"], START["eta"], START["sigma"], START["rho"],
                                 START["V_0"], M1, M2, N, theta, grids, U_0, market, max_iter=3, tol=1e-12, scheme=H.SCHEME_MCS)
    assert res["iterations"] == 3 and len(res["history"]) == 3
    assert [c[0] for c in sv.calls] == ["jac", "base"] * 3
    assert all(c[1] == 2 for c in sv.calls), sv.calls
    assert res["history"][-1]["error"] < res["history"][0]["error"]  # the loop ran on these prices and moved towards the market
    # the prices are the scheme's: Douglas at the same theta prices the start differently
    first = sv._prices(Cm.S_0, START["V_0"], Cm.R_D, Cm.R_F, START["rho"], START["sigma"], START["kappa"], START["eta"], M1, M2,
                       theta, steps, grids, U_0, S.MCS)
    assert res["history"][0]["error"] == pytest.approx(float(np.sum((market - first) ** 2)), rel=1e-12)
    douglas = sv._prices(Cm.S_0, START["V_0"], Cm.R_D, Cm.R_F, START["rho"], START["sigma"], START["kappa"], START["eta"], M1, M2,
                         theta, steps, grids, U_0, S.DOUGLAS)
    assert np.abs(douglas - first).max() > 1e-6


def test_multi_maturity_driver_hands_the_scheme_on():
    strikes = [95.0, 105.0]
    points = Cal.make_calibration_points(strikes, [0.1, 0.2], steps_per_year=20, min_steps=2)
    grids, U_0 = _setup([p.strike for p in points])
    sv = SchemeOracleSolver()
    market = np.full(len(points), 5.0)
    Cal.calibrate_european_multi_maturity(sv, Cm.S_0, Cm.R_D, Cm.R_F, START["kappa"], START["eta"], START["sigma"], START["rho"],
                                          START["V_0"], M1, M2, 0.5, points, grids, U_0, market, max_iter=1, tol=1e-12, delta_tol=1e-12,
                                          scheme=H.SCHEME_CRAIG_SNEYD)
    assert sv.calls == [("jac_mm", 1), ("base_mm", 1)]


@pytest.mark.parametrize("driver,extra", [(Cal.calibrate_american, ()), (Cal.calibrate_dividends, (H.Dividends(*Cm.DIVS),)),
                                          (Cal.calibrate_american_dividends, (H.Dividends(*Cm.DIVS),))])
def test_other_variants_refuse_a_scheme_before_any_solve(driver, extra):
    grids, U_0 = _setup()

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("launcher %s called" % name)

    with pytest.raises(ValueError):
        driver(Untouched(), Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, START["kappa"], START["eta"], START["sigma"], START["rho"], START["V_0"],
               M1, M2, N, 0.5, grids, U_0, np.zeros(len(STRIKES)), *extra, scheme=2)
    points = Cal.make_calibration_points(STRIKES, [0.2], min_steps=2)
    with pytest.raises(ValueError):
        Cal.calibrate_american_dividends_multi_maturity(Untouched(), Cm.S_0, Cm.R_D, Cm.R_F, START["kappa"], START["eta"], START["sigma"],
                                                        START["rho"], START["V_0"], M1, M2, 0.5, points, grids, U_0,
                                                        np.zeros(len(STRIKES)), H.Dividends(*Cm.DIVS), scheme=3)


def test_without_a_scheme_the_launchers_are_called_as_before():
    """common.OracleSolver's launchers take no `scheme`: the drivers must not pass one when it is left out (or 0)."""
    grids, U_0 = _setup()
    sv = Cm.OracleSolver()
    p = O.make_params(M1, M2, N, Cm.T / N, 0.5, Cm.R_D, Cm.R_F, TRUE["rho"], TRUE["sigma"], TRUE["kappa"], TRUE["eta"], O.EU)
    market = O.base_prices(p, Cm.S_0, TRUE["v0"], grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U_0)[0]
    args = (sv, Cm.S_0, Cm.T, Cm.R_D, Cm.R_F, START["kappa"], START["eta"], START["sigma"], START["rho"], START["V_0"], M1, M2, N, 0.5,
            grids, U_0, market)
    a = Cal.calibrate_european(*args, max_iter=2, tol=1e-12)
    b = Cal.calibrate_european(*args, max_iter=2, tol=1e-12, scheme=0)
    assert a["iterations"] == 2 and a["history"][1]["params"] == b["history"][1]["params"]
    # ... and the scheme-aware stand-in then sees scheme 0 in every call
    sv2 = SchemeOracleSolver()
    c = Cal.calibrate_european(sv2, *args[1:], max_iter=2, tol=1e-12)
    assert c["iterations"] == 2 and len(sv2.calls) == 4 and all(s == 0 for _, s in sv2.calls)
