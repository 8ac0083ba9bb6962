"""Levenberg-Marquardt calibration of (kappa, eta, sigma, rho, v0) on top of the batched solver: the host loops of
the reference's calibration drivers (src/heston_calibration.cpp) with the same update, clamps, accept/reject rule
and lambda schedule, made rank-aware: every rank owns a contiguous shard of the calibration instruments, and the
normal equations are all-reduced (31 doubles per iteration, 1 double for the trial error).

    calibrate_european                          test_calibration_european                          :26-512
    calibrate_american                          test_calibration_american                          :515-1033
    calibrate_dividends                         test_calibration_dividends                         :1036-1585
    calibrate_american_dividends                test_calibration_american_dividends                :1588-2160
    calibrate_european_multi_maturity           test_calibration_european_multi_maturity           :2428-2933
    calibrate_american_dividends_multi_maturity test_calibration_american_divident_multi_maturity  :3245-3820
    calibrate_bermudan                          no counterpart: European / dividend sweeps with exercise on chosen steps
    calibrate_european_maturity_ladder          no counterpart: all maturities of a strike from ONE sweep on a shared delta_t
    calibrate_bates, calibrate_bates_jumps      no counterpart: the Bates model, the jump law held fixed / fitted (8 parameters)
    calibrate_bates_surface                     no counterpart: a Bates strike x maturity surface from ONE sweep per parameter group

`solver` is anything with the mirrored launchers of solver.HestonADI (`compute_jacobian*`, `compute_base_prices*`).
"""
import collections
import math

import numpy as np

from . import market as _market
from . import solver as _solver
from .distributed import Communicator

RHO_MIN, RHO_MAX = -1.0, 1.0           # heston_calibration.cpp:194
KAPPA_FLOOR, OTHER_FLOOR = 1e-3, 1e-2  # heston_calibration.cpp:286-290
LAMBDA_MIN, LAMBDA_MAX = 1e-7, 1e7     # heston_calibration.cpp:398-408
# The jump law of calibrate_bates_jumps (no counterpart).  The floor of the intensity keeps the mu_J and sigma_J columns of the
# Jacobian from vanishing (they scale with it: zero pivots); its ceiling is JUMP_INTENSITY_CEIL / delta_t, so that (intensity + eps)
# delta_t stays admissible.
JUMP_INTENSITY_FLOOR, JUMP_INTENSITY_CEIL = 1e-3, 0.99
JUMP_MEAN_MIN, JUMP_MEAN_MAX = -1.0, 1.0
JUMP_VOL_FLOOR, JUMP_VOL_MAX = OTHER_FLOOR, 1.0

EU, AM, DIV, AM_DIV = _solver.EU, _solver.AM, _solver.DIV, _solver.AM_DIV

# heston_calibration.cpp:2165-2171
CalibrationPoint = collections.namedtuple("CalibrationPoint", "strike maturity time_steps delta_t global_index")


def make_calibration_points(strikes, maturities, steps_per_year=20, min_steps=20):
    """Flat strike-fastest list, N_m = max(20, int(20 T_m)), dt_m = T_m / N_m (heston_calibration.cpp:2512-2531)."""
    pts = []
    for m, T_m in enumerate(maturities):
        N_m = max(min_steps, int(T_m * steps_per_year))
        dt_m = T_m / N_m
        for s, K in enumerate(strikes):
            pts.append(CalibrationPoint(float(K), float(T_m), N_m, dt_m, m * len(strikes) + s))
    return pts


def make_ladder_points(strikes, maturities, delta_t):
    """The points of a maturity ladder, flat and strike-fastest like make_calibration_points (global_index = m * len(strikes) +
    s), but on ONE delta_t: time_steps = T_m / delta_t.  Raises ValueError unless every maturity is a whole number (>= 1) of
    steps of delta_t, to within 1e-9 steps, and the maturities are strictly increasing.  This is NOT the reference's convention
    (N_m = max(20, int(20 T_m)), dt_m = T_m / N_m): the maturities of a ladder share the step, so one sweep per strike passes
    through all of them."""
    if not (delta_t > 0 and math.isfinite(delta_t)):
        raise ValueError("delta_t must be positive")
    steps = []
    for T_m in maturities:
        x = T_m / delta_t
        n = int(round(x))
        if n < 1 or abs(x - n) > 1e-9:
            raise ValueError("maturity %r is %.12g steps of delta_t = %r: not a whole number of steps" % (T_m, x, delta_t))
        if steps and n <= steps[-1]:
            raise ValueError("the maturities of a ladder must be strictly increasing (%r after %d steps)" % (T_m, steps[-1]))
        steps.append(n)
    if not steps:
        raise ValueError("no maturities")
    return [CalibrationPoint(float(K), float(T_m), n, float(delta_t), m * len(strikes) + s)
            for m, (T_m, n) in enumerate(zip(maturities, steps)) for s, K in enumerate(strikes)]


def clamp_parameters(kappa, eta, sigma, rho, v0):
    return (max(KAPPA_FLOOR, kappa), max(OTHER_FLOOR, eta), max(OTHER_FLOOR, sigma),
            min(RHO_MAX, max(RHO_MIN, rho)), max(OTHER_FLOOR, v0))


def clamp_jump_parameters(jump_intensity, jump_mean, jump_vol, delta_t):
    """The clamps of the three jump parameters of calibrate_bates_jumps, beside clamp_parameters' five."""
    return (min(JUMP_INTENSITY_CEIL / delta_t, max(JUMP_INTENSITY_FLOOR, jump_intensity)),
            min(JUMP_MEAN_MAX, max(JUMP_MEAN_MIN, jump_mean)), min(JUMP_VOL_MAX, max(JUMP_VOL_FLOOR, jump_vol)))


class _WS:  # minimal DO_Workspace: the launchers read the initial condition from .U
    pass


def _launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, grids, U_0, dividends, points, scheme=0):
    """Two closures (params -> (J, base)), (params -> trial prices) over the launcher pair of the variant.  `scheme` (0 Douglas,
    1 Craig-Sneyd, 2 Modified Craig-Sneyd, 3 Hundsdorfer-Verwer) goes to every call of the European pairs; 0 calls the
    launchers without it, as before the schemes existed."""
    n_loc = grids.Vec_s.shape[0]
    total_size = (m1 + 1) * (m2 + 1)
    if scheme and variant != EU:
        raise ValueError("scheme %r: the predictor-corrector schemes price European options only (variant %r)" % (scheme, variant))
    sch = {"scheme": scheme} if scheme else {}
    if variant in (DIV, AM_DIV) and dividends is None:
        raise ValueError("this variant needs a dividend schedule")

    def workspace():
        ws = _WS()
        ws.U = _clone(U_0)                                               # deep_copy(workspace.U, U_0)
        return ws

    if points is not None:                                               # multi-maturity launchers
        if variant == EU:
            def jac(k, e, s, r, v, eps):
                return solver.compute_jacobian_multi_maturity(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, theta,
                                                              points, n_loc, grids, U_0, eps=eps, **sch)

            def base(k, e, s, r, v):
                return solver.compute_base_prices_multi_maturity(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size,
                                                                 theta, points, n_loc, grids, workspace(), **sch)
        elif variant == AM_DIV:
            def jac(k, e, s, r, v, eps):
                return solver.compute_jacobian_multi_maturity_american_dividends(
                    S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, theta, points, n_loc, grids, U_0, dividends,
                    eps=eps)

            def base(k, e, s, r, v):
                return solver.compute_base_prices_multi_maturity_american_dividends(
                    S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, theta, points, n_loc, grids, U_0, workspace(),
                    dividends)
        else:
            raise ValueError("the reference has multi-maturity launchers for EU and AM_DIV only")
        return jac, base

    delta_t = T / N
    head = lambda k, e, s, r, v: (S_0, v, T, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc, grids)
    if variant == EU:
        jac = lambda k, e, s, r, v, eps: solver.compute_jacobian(*head(k, e, s, r, v), U_0, eps=eps, **sch)
        base = lambda k, e, s, r, v: solver.compute_base_prices(*head(k, e, s, r, v), workspace(), **sch)
    elif variant == AM:
        jac = lambda k, e, s, r, v, eps: solver.compute_jacobian_american(*head(k, e, s, r, v), U_0, eps=eps)
        base = lambda k, e, s, r, v: solver.compute_base_prices_american(*head(k, e, s, r, v), U_0, workspace())
    elif variant == DIV:
        jac = lambda k, e, s, r, v, eps: solver.compute_jacobian_dividends(*head(k, e, s, r, v), U_0, dividends, eps=eps)
        base = lambda k, e, s, r, v: solver.compute_base_prices_dividends(*head(k, e, s, r, v), workspace(), dividends)
    elif variant == AM_DIV:
        jac = lambda k, e, s, r, v, eps: solver.compute_jacobian_american_dividends(*head(k, e, s, r, v), U_0, dividends,
                                                                                    eps=eps)
        base = lambda k, e, s, r, v: solver.compute_base_prices_american_dividends(*head(k, e, s, r, v), U_0, workspace(),
                                                                                   dividends)
    else:
        raise ValueError("unknown variant %r" % (variant,))
    return jac, base


def calibrate(solver, variant, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
              market_prices, dividends=None, calibration_points=None, max_iter=20, tol=0.1, delta_tol=None, eps=1e-6,
              lam=0.01, comm=None, lm_partials=_solver.lm_partials, lm_solve=_solver.lm_solve, scheme=0, launchers=None,
              extra=(), clamp_extra=None, solves_per_iteration=7):
    """The LM loop shared by all drivers (heston_calibration.cpp:204-417).  `grids`, `U_0`, `market_prices` (and
    `calibration_points` for the multi-maturity drivers, which then ignore T and N) are this rank's shard.
    `scheme`: the time stepper of every Jacobian and trial-price solve of the loop (0 Douglas, 1 Craig-Sneyd, 2 Modified
    Craig-Sneyd, 3 Hundsdorfer-Verwer), European variant only (ValueError otherwise, before any solve); `theta` is the scheme's:
    the usual pairs are 1/3 for MCS and 1/2 + sqrt(3)/6 for HV, which are second order in time where Douglas is first.
    `launchers`: the pair of closures _launchers would build, for drivers whose instruments are not one instance each (the
    maturity ladder); market_prices then follow the closures' order.
    `extra`: further parameters behind the five (calibrate_bates_jumps: the jump law) -- the closures then take 5 + len(extra)
    parameters, the Jacobian has as many columns, and `clamp_extra` (a function of the extra entries that returns them clamped;
    None: none) stands beside clamp_parameters.  The result then carries "extra".  `solves_per_iteration`: sweeps per instance and
    iteration, for `pde_solves` (columns + 1 for the Jacobian, 1 for the trial).
    Stops when ||delta||_2 < delta_tol (default: tol) or sum r^2 < tol.  Returns a dict with the calibrated
    parameters, final error, iteration count, PDE-solve count, the last computed model prices and the trajectory."""
    comm = comm or Communicator()
    n_loc = grids.Vec_s.shape[0]
    delta_tol = tol if delta_tol is None else delta_tol
    market = np.asarray(market_prices, dtype=np.float64)
    jac, base_fn = launchers or _launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, grids, U_0, dividends,
                                           calibration_points, scheme=scheme)
    extra = tuple(float(e) for e in extra)
    cur = (kappa, eta, sigma, rho, V_0) + extra
    final_error, iteration_count, converged = 100.0, 0, False
    history = []
    model = None

    # Device-resident shards (CUDA tensors through a real handle): the Jacobian rows and prices stay in HBM and
    # J^T J / J^T r / sum r^2 are reduced there (hadi_lm_partials_device) -- 31 doubles per iteration leave the GPU, as
    # after the reference's KokkosBlas gemm/gemv (jacobian_computation.cpp:117,154).  Host arrays take the host loop.
    on_device = _solver._is_device(U_0) and hasattr(solver, "_h") and lm_partials is _solver.lm_partials
    market_d = None
    if on_device:
        import torch
        market_d = torch.from_numpy(np.ascontiguousarray(market)).to(U_0.device)

    for it in range(max_iter):
        J, base = jac(*cur, eps)
        model = base
        if on_device:
            part_loc = _solver.lm_partials_device(solver, J, base, market_d)
        else:
            J, base = _to_numpy(J), _to_numpy(base)
            model = base
            resid = market - base                                        # heston_calibration.cpp:271-275
            part_loc = lm_partials(J, resid)
        part = comm.allreduce_sum(part_loc)                              # the only collective of the step
        delta = lm_solve(part, lam)
        moved = tuple(c + d for c, d in zip(cur, delta))
        new = clamp_parameters(*moved[:5])
        if extra:
            new = new + tuple(clamp_extra(*moved[5:]) if clamp_extra else moved[5:])
        delta_norm = float(np.sqrt(np.sum(delta * delta)))
        current_error = float(part[-1])                                  # sum r^2: the last slot, whatever the width
        history.append({"iter": it + 1, "params": cur, "error": current_error, "lambda": lam,
                        "delta": delta.copy(), "trial": new})
        if delta_norm < delta_tol or current_error < tol:                # heston_calibration.cpp:322-338
            converged = True
            cur = new
            final_error = current_error
            iteration_count = it + 1
            break
        trial = base_fn(*new)
        model = trial
        if on_device:
            solver.wait_stream()  # (trial is complete; torch ops below run on torch's stream)
            loc_err = float(((market_d - trial) ** 2).sum().item())      # one double leaves the GPU
        else:
            trial = _to_numpy(trial)
            model = trial
            r_new = market - trial
            loc_err = float(np.sum(r_new * r_new))
        new_error = float(comm.allreduce_sum(np.array([loc_err]))[0])
        history[-1]["trial_error"] = new_error
        if new_error < current_error:                                    # heston_calibration.cpp:398-408
            cur = new
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = min(lam * 10.0, LAMBDA_MAX)
        final_error = min(new_error, current_error)
        iteration_count = it + 1
    n_glob = int(round(comm.allreduce_sum(np.array([float(n_loc)]))[0]))
    out = {"kappa": cur[0], "eta": cur[1], "sigma": cur[2], "rho": cur[3], "v0": cur[4],
           "final_error": final_error, "iterations": iteration_count, "converged": converged,
           "pde_solves": n_glob * solves_per_iteration * iteration_count - n_glob,  # heston_calibration.cpp:428
           "initial": (kappa, eta, sigma, rho, V_0), "model_prices": None if model is None else _to_numpy(model),
           "history": history}
    if extra:
        out["extra"] = cur[5:]
    return out


def calibrate_european(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                       market_prices, max_iter=15, tol=0.1, scheme=0, **kw):
    """scheme / theta: see calibrate (e.g. scheme=2, theta=1/3: Modified Craig-Sneyd)."""
    return calibrate(solver, EU, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                     market_prices, max_iter=max_iter, tol=tol, scheme=scheme, **kw)


def calibrate_american(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                       market_prices, max_iter=15, tol=0.1, **kw):
    return calibrate(solver, AM, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                     market_prices, max_iter=max_iter, tol=tol, **kw)


def calibrate_dividends(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                        market_prices, dividends, max_iter=20, tol=0.1, **kw):
    return calibrate(solver, DIV, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                     market_prices, dividends=dividends, max_iter=max_iter, tol=tol, **kw)


def calibrate_american_dividends(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                                 market_prices, dividends, max_iter=20, tol=0.1, **kw):
    return calibrate(solver, AM_DIV, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0,
                     market_prices, dividends=dividends, max_iter=max_iter, tol=tol, **kw)


def multi_maturity_tolerances(n_points):
    """tol = 0.1 sqrt(n), delta_tol = 0.1 (1 + ln n): heston_calibration.cpp:2544-2545."""
    return 1e-1 * math.sqrt(n_points), 1e-1 * (1.0 + math.log(n_points))


def calibrate_european_multi_maturity(solver, S_0, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, theta,
                                      calibration_points, grids, U_0, market_prices, max_iter=15, tol=None,
                                      delta_tol=None, n_total=None, scheme=0, **kw):
    """`n_total` = global number of calibration points (defaults to this rank's, i.e. single rank).  scheme / theta: see
    calibrate."""
    t, dtol = multi_maturity_tolerances(n_total or len(calibration_points))
    return calibrate(solver, EU, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0,
                     market_prices, calibration_points=calibration_points, max_iter=max_iter,
                     tol=t if tol is None else tol, delta_tol=dtol if delta_tol is None else delta_tol, scheme=scheme, **kw)


def _ladder_launchers(solver, S_0, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, scheme=0):
    """The closures of calibrate() over the ladder launchers: one instance per strike, residual rows in the order
    m * len(strikes) + s of the multi-maturity drivers (the launchers return [strike][maturity])."""
    n_s = grids.Vec_s.shape[0]
    total_size = (m1 + 1) * (m2 + 1)
    N = int(snap_steps[-1])
    sch = {"scheme": scheme} if scheme else {}

    def by_maturity(x):  # [n_s][n_m][...] -> [n_m * n_s][...], numpy or torch
        y = x.transpose(0, 1) if hasattr(x, "detach") else np.swapaxes(x, 0, 1)
        y = y.contiguous() if hasattr(y, "contiguous") else np.ascontiguousarray(y)
        return y.reshape((-1,) + tuple(x.shape[2:]))

    def jac(k, e, s, r, v, eps):
        J, base = solver.compute_jacobian_ladder(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_s, grids,
                                                 U_0, snap_steps, eps=eps, **sch)
        return by_maturity(J), by_maturity(base)

    def base(k, e, s, r, v):
        ws = _WS()
        ws.U = _clone(U_0)
        return by_maturity(solver.compute_base_prices_ladder(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t,
                                                             n_s, grids, ws, snap_steps, **sch))

    return jac, base


def calibrate_european_maturity_ladder(solver, S_0, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, theta, strikes, maturities,
                                       delta_t, grids, U_0, market_prices, max_iter=15, tol=None, delta_tol=None, n_total=None,
                                       scheme=0, **kw):
    """calibrate_european_multi_maturity on a maturity ladder: `grids` / `U_0` hold ONE instance per strike (this rank's
    strikes), every maturity is a whole number of steps of the shared delta_t (make_ladder_points raises otherwise), and each LM
    iteration runs max(n_m) steps per strike and parameter group where the per-maturity batch runs sum(n_m).  market_prices:
    [len(maturities) * len(strikes)] in the order m * len(strikes) + s, as the residuals.  Same discretisation as
    calibrate_european_multi_maturity fed make_ladder_points -- the prices agree bit for bit on the same execution path, so the
    LM iterates are the same.  r_f must be 0 (the library refuses a ladder of calls otherwise, hadi.h).  `pde_solves` counts the
    sweeps actually run (one per strike and group).  scheme / theta: see calibrate.
    Measured on one MI355X (profiles/ladder_ab.txt), Jacobian / base prices of the per-maturity launchers
    -> the ladder's, ms per call: it was faster on every surface measured -- 50x25 with 10 evenly spaced maturities (10 .. 100
    steps), 500 strikes 16.2 -> 3.5 / 3.2 -> 1.2 and 50 strikes 2.0 -> 1.2 / 1.29 -> 1.03 (there the per-maturity batch was
    filling idle CUs: 1.2 - 1.7x where sum n_k / max n_k is 5.5); 256x128 with 64 strikes x 8 maturities 41.8 -> 8.4 / 10.2 ->
    3.1.  Smaller surfaces than 50 strikes were not measured."""
    pts = make_ladder_points(strikes, maturities, delta_t)
    n_s, n_m = len(strikes), len(maturities)
    if grids.Vec_s.shape[0] != n_s:
        raise ValueError("a maturity ladder takes one grid per strike (%d grids, %d strikes)" % (grids.Vec_s.shape[0], n_s))
    market = np.asarray(market_prices, dtype=np.float64).reshape(-1)
    if market.size != n_s * n_m:
        raise ValueError("market_prices must hold len(maturities) * len(strikes) prices, maturity by maturity")
    snap_steps = [pts[m * n_s].time_steps for m in range(n_m)]
    t, dtol = multi_maturity_tolerances(n_total or len(pts))
    launch = _ladder_launchers(solver, S_0, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, scheme=scheme)
    return calibrate(solver, EU, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0, market,
                     max_iter=max_iter, tol=t if tol is None else tol, delta_tol=dtol if delta_tol is None else delta_tol,
                     scheme=scheme, launchers=launch, **kw)


def _surface_launchers(solver, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, spots, scales, scheme=0):
    """The closures of calibrate() over the sample launchers: ONE instance, whose [1][maturity][strike] outputs are already in the
    residual order m * len(strikes) + s."""
    total_size = (m1 + 1) * (m2 + 1)
    N = int(snap_steps[-1])
    sch = {"scheme": scheme} if scheme else {}

    def jac(k, e, s, r, v, eps):
        J, base = solver.compute_jacobian_samples(spots, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, 1, grids,
                                                  U_0, snap_steps, scales=scales, eps=eps, **sch)
        return J.reshape(-1, 5), base.reshape(-1)

    def base(k, e, s, r, v):
        ws = _WS()
        ws.U = _clone(U_0)
        return solver.compute_base_prices_samples(spots, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, 1, grids,
                                                  ws, snap_steps, scales=scales, **sch).reshape(-1)

    return jac, base


def calibrate_european_surface(solver, S_0, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, theta, base_strike, strikes, maturities,
                               delta_t, grids, U_0, market_prices, max_iter=15, tol=None, delta_tol=None, n_total=None, scheme=0,
                               **kw):
    """calibrate_european_maturity_ladder with the strikes taken out of the batch as well: `grids` / `U_0` hold ONE instance, built
    at `base_strike`, and every strike of every maturity is read off its sweep through strike_samples (the homogeneity of the Heston
    problem in (s, K); solver.strike_samples states the claim and its limits) -- six sweeps per Jacobian and one per trial,
    whatever the number of strikes, so the instance can afford a finer grid.  `strikes` are this rank's strikes (the partial-sum
    all-reduce shards the rows as before); every maturity is a whole number of steps of delta_t (make_ladder_points raises
    otherwise).  market_prices: [len(maturities) * len(strikes)] in the order m * len(strikes) + s, as the residuals.  S_0 K / K'
    must lie on the base grid for every strike K' (HadiError, status 4, otherwise).  r_f must be 0 for calls (the ladder's rule).
    `pde_solves` counts the sweeps actually run: six per Jacobian and one per trial.  The prices are those of the grid scaled per
    strike, not of GridViewsBatch.for_strikes' grids: on the oracle the two differ by 1.5e-2 / 2.7e-3 / 1.1e-3 on 50x25 / 100x50 /
    200x100 (strikes 80 .. 125 around K = 100), inside the grids' own discretisation error (4.4e-2 / 1.6e-2 / 1.1e-2 against the
    semi-analytic price).
    Measured on one MI355X (DESIGN.md "Sampled ladder", profiles/surface_ab.txt), ms per call, 10 maturities (10 .. 100 steps), the
    ladder launchers with one 50x25 instance per strike -> this driver's launchers with one instance on 50x25 / 100x50 / 200x100:
    500 strikes, Jacobian 3.72 -> 1.06 / 1.30 / 1.58 and base prices 1.26 -> 1.03 / 1.26 / 1.46; 50 strikes, Jacobian 1.26 -> 1.04 /
    1.21 / 1.47 and base prices 1.03 -> 1.02 / 1.18 / 1.37.  It loses wherever the ladder call is already at its fixed cost of about
    1 ms: the base-price calls on the finer grids and the 50-strike Jacobian on 200x100."""
    pts = make_ladder_points(strikes, maturities, delta_t)
    n_s, n_m = len(strikes), len(maturities)
    if grids.Vec_s.shape[0] != 1:
        raise ValueError("a surface takes ONE grid, built at base_strike (%d grids)" % grids.Vec_s.shape[0])
    market = np.asarray(market_prices, dtype=np.float64).reshape(-1)
    if market.size != n_s * n_m:
        raise ValueError("market_prices must hold len(maturities) * len(strikes) prices, maturity by maturity")
    spots, scales = _solver.strike_samples(S_0, base_strike, strikes)
    snap_steps = [pts[m * n_s].time_steps for m in range(n_m)]
    t, dtol = multi_maturity_tolerances(n_total or len(pts))
    launch = _surface_launchers(solver, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, spots, scales, scheme=scheme)
    return calibrate(solver, EU, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0, market,
                     max_iter=max_iter, tol=t if tol is None else tol, delta_tol=dtol if delta_tol is None else delta_tol,
                     scheme=scheme, launchers=launch, **kw)


def _bermudan_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, schedule, grids, U_0, dividends, scheme=0):
    """The closures of calibrate() over the Bermudan launchers: one instance per strike, as the single-maturity drivers."""
    n_loc = grids.Vec_s.shape[0]
    total_size = (m1 + 1) * (m2 + 1)
    delta_t = T / N
    kw = {"variant": variant, "dividends": dividends}
    if scheme:
        kw["scheme"] = scheme

    def jac(k, e, s, r, v, eps):
        return solver.compute_jacobian_bermudan(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc, grids,
                                                U_0, schedule, eps=eps, **kw)

    def base(k, e, s, r, v):
        ws = _WS()
        ws.U = _clone(U_0)
        return solver.compute_base_prices_bermudan(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc,
                                                   grids, ws, schedule, **kw)

    return jac, base


def calibrate_bermudan(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                       exercise_steps, dividends=None, max_iter=15, tol=0.1, scheme=0, **kw):
    """calibrate_european / calibrate_dividends on Bermudan quotes: every Jacobian and trial-price solve is the European sweep
    (with `dividends`: the dividend sweep) with exercise at the end of the steps `exercise_steps` -- a list shared by the
    strikes, or one list per strike (solver.exercise_steps maps calendar dates to steps).  U_0 is the payoff.  scheme / theta:
    see calibrate (without dividends only)."""
    variant = DIV if dividends is not None and len(dividends) else EU
    if scheme and variant != EU:
        raise ValueError("scheme %r: the predictor-corrector schemes price European sweeps only" % (scheme,))
    launch = _bermudan_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, exercise_steps, grids, U_0,
                                 dividends if variant == DIV else None, scheme=scheme)
    return calibrate(solver, variant, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                     dividends=dividends, max_iter=max_iter, tol=tol, scheme=scheme, launchers=launch, **kw)


def _bates_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, jumps, grids, U_0, dividends, scheme=0):
    """The closures of calibrate() over the Bates launchers: one instance per strike, the jump parameters held fixed."""
    n_loc = grids.Vec_s.shape[0]
    total_size = (m1 + 1) * (m2 + 1)
    delta_t = T / N
    kw = {"variant": variant, "dividends": dividends}
    if scheme:
        kw["scheme"] = scheme

    def jac(k, e, s, r, v, eps):
        return solver.compute_jacobian_bates(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc, grids,
                                             U_0, *jumps, eps=eps, **kw)

    def base(k, e, s, r, v):
        ws = _WS()
        ws.U = _clone(U_0)
        return solver.compute_base_prices_bates(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc,
                                                grids, ws, *jumps, **kw)

    return jac, base


def calibrate_bates(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                    jump_intensity, jump_mean, jump_vol, shared_grid=False, dividends=None, max_iter=15, tol=0.1, scheme=0, **kw):
    """calibrate_european / calibrate_dividends under the Bates model: every Jacobian and trial-price solve is the European sweep
    (with `dividends`: the dividend sweep) with the lognormal-jump sub-step at the end of every step.  The five Heston parameters
    are fitted; the jump parameters (a scalar or one value per strike each) are inputs and stay fixed.  shared_grid: see
    HestonADI.bates_timestepping.  scheme / theta: see calibrate (without dividends only)."""
    variant = DIV if dividends is not None and len(dividends) else EU
    if scheme and variant != EU:
        raise ValueError("scheme %r: the predictor-corrector schemes price European sweeps only" % (scheme,))
    launch = _bates_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, (jump_intensity, jump_mean, jump_vol, shared_grid),
                              grids, U_0, dividends if variant == DIV else None, scheme=scheme)
    return calibrate(solver, variant, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                     dividends=dividends, max_iter=max_iter, tol=tol, scheme=scheme, launchers=launch, **kw)


def _bates_jumps_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, shared_grid, grids, U_0, dividends, scheme=0):
    """The closures of calibrate() over the eight-column Bates launchers: one instance per strike, eight parameters."""
    n_loc = grids.Vec_s.shape[0]
    total_size = (m1 + 1) * (m2 + 1)
    delta_t = T / N
    kw = {"variant": variant, "dividends": dividends}
    if scheme:
        kw["scheme"] = scheme

    def jac(k, e, s, r, v, lj, mj, sj, eps):
        return solver.compute_jacobian_bates_jumps(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc, grids,
                                                   U_0, lj, mj, sj, shared_grid, eps=eps, **kw)

    def base(k, e, s, r, v, lj, mj, sj):
        ws = _WS()
        ws.U = _clone(U_0)
        return solver.compute_base_prices_bates(S_0, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, n_loc,
                                                grids, ws, lj, mj, sj, shared_grid, **kw)

    return jac, base


def calibrate_bates_jumps(solver, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                          jump_intensity, jump_mean, jump_vol, shared_grid=False, dividends=None, max_iter=15, tol=0.1, scheme=0, **kw):
    """calibrate_bates with the jump law fitted too: eight parameters -- the five of calibrate_bates and the scalars jump_intensity,
    jump_mean, jump_vol, which are the start values.  Every iteration is one eight-column Jacobian (compute_jacobian_bates_jumps:
    nine sweeps per strike) and one trial (compute_base_prices_bates); 73 doubles are all-reduced.  Clamps beside clamp_parameters:
    clamp_jump_parameters.  The result carries jump_intensity, jump_mean and jump_vol beside calibrate's keys; `pde_solves` counts
    ten sweeps per strike and iteration.  shared_grid, dividends, scheme / theta: as calibrate_bates."""
    for x, name in ((jump_intensity, "jump_intensity"), (jump_mean, "jump_mean"), (jump_vol, "jump_vol")):
        if np.ndim(x) != 0:
            raise ValueError("%s: calibrate_bates_jumps fits one jump law, so a scalar start value" % name)
    variant = DIV if dividends is not None and len(dividends) else EU
    if scheme and variant != EU:
        raise ValueError("scheme %r: the predictor-corrector schemes price European sweeps only" % (scheme,))
    delta_t = T / N
    launch = _bates_jumps_launchers(solver, variant, S_0, T, r_d, r_f, m1, m2, N, theta, shared_grid, grids, U_0,
                                    dividends if variant == DIV else None, scheme=scheme)
    res = calibrate(solver, variant, S_0, T, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, N, theta, grids, U_0, market_prices,
                    dividends=dividends, max_iter=max_iter, tol=tol, scheme=scheme, launchers=launch,
                    extra=(jump_intensity, jump_mean, jump_vol), clamp_extra=lambda lj, mj, sj: clamp_jump_parameters(lj, mj, sj, delta_t),
                    solves_per_iteration=10, **kw)
    res["jump_intensity"], res["jump_mean"], res["jump_vol"] = res.pop("extra")
    return res


def _bates_surface_launchers(solver, variant, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, spots, scales, jumps, dividends,
                             scheme=0):
    """The closures of calibrate() over the Bates sample launchers: ONE instance, whose [1][maturity][strike] outputs are already in
    the residual order m * len(strikes) + s.  jumps: None = the jump law is fitted (eight parameters, the closures take it behind
    the five), else the fixed (jump_intensity, jump_mean, jump_vol)."""
    total_size = (m1 + 1) * (m2 + 1)
    N = int(snap_steps[-1])
    kw = {"scales": scales, "variant": variant, "dividends": dividends}
    if scheme:
        kw["scheme"] = scheme

    def jac(k, e, s, r, v, *rest):
        law, eps = (rest[:3], rest[3]) if jumps is None else (jumps, rest[0])
        J, base = solver.compute_jacobian_bates_samples(spots, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, 1, grids,
                                                        U_0, snap_steps, *law, jump_columns=jumps is None, eps=eps, **kw)
        return J.reshape(-1, 8 if jumps is None else 5), base.reshape(-1)

    def base(k, e, s, r, v, *rest):
        ws = _WS()
        ws.U = _clone(U_0)
        return solver.compute_base_prices_bates_samples(spots, v, r_d, r_f, r, s, k, e, m1, m2, total_size, N, theta, delta_t, 1, grids,
                                                        ws, snap_steps, *(rest if jumps is None else jumps), **kw).reshape(-1)

    return jac, base


def calibrate_bates_surface(solver, S_0, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, theta, base_strike, strikes, maturities,
                            delta_t, grids, U_0, market_prices, jump_intensity, jump_mean, jump_vol, fit_jumps=True, dividends=None,
                            max_iter=15, tol=None, delta_tol=None, n_total=None, scheme=0, **kw):
    """calibrate_european_surface under the Bates model: `grids` / `U_0` hold ONE instance, built at `base_strike`, and every strike
    of every maturity is read off its sweep through strike_samples.  Jumps are multiplicative, so the Bates problem is as
    homogeneous in (s, K) as Heston's (the generator of the jump term depends on the s-grid through ratios only); with `dividends`
    only PROPORTIONAL ones keep that, as strike_samples says of cash amounts.  A jump law is identified by the short-dated skew
    ACROSS maturities, which is what this driver fits and a single-maturity driver cannot.
    fit_jumps True: eight parameters -- the five and the scalars jump_intensity, jump_mean, jump_vol, which are the start values;
    every iteration is one eight-column Jacobian (compute_jacobian_bates_samples: nine sweeps) and one trial
    (compute_base_prices_bates_samples); 73 doubles are all-reduced; clamps beside clamp_parameters: clamp_jump_parameters with
    this delta_t; the result carries jump_intensity, jump_mean, jump_vol.  fit_jumps False: the law is held fixed and the loop is
    the five-column one (six sweeps and one).  `pde_solves` counts the sweeps actually run.  market_prices:
    [len(maturities) * len(strikes)] in the order m * len(strikes) + s.  r_f must be 0 for calls (the ladder's rule); every
    maturity is a whole number of steps of delta_t.  scheme / theta: see calibrate (without dividends only).
    Measured on one MI355X: profiles/bates_surface_ab.txt (this driver's launchers against one compute_jacobian_bates_jumps /
    compute_base_prices_bates call per maturity, and the two routes of the new call against each other)."""
    for x, name in ((jump_intensity, "jump_intensity"), (jump_mean, "jump_mean"), (jump_vol, "jump_vol")):
        if np.ndim(x) != 0:
            raise ValueError("%s: calibrate_bates_surface takes one jump law, so a scalar" % name)
    pts = make_ladder_points(strikes, maturities, delta_t)
    n_s, n_m = len(strikes), len(maturities)
    if grids.Vec_s.shape[0] != 1:
        raise ValueError("a surface takes ONE grid, built at base_strike (%d grids)" % grids.Vec_s.shape[0])
    market = np.asarray(market_prices, dtype=np.float64).reshape(-1)
    if market.size != n_s * n_m:
        raise ValueError("market_prices must hold len(maturities) * len(strikes) prices, maturity by maturity")
    variant = DIV if dividends is not None and len(dividends) else EU
    if scheme and variant != EU:
        raise ValueError("scheme %r: the predictor-corrector schemes price European sweeps only" % (scheme,))
    spots, scales = _solver.strike_samples(S_0, base_strike, strikes)
    snap_steps = [pts[m * n_s].time_steps for m in range(n_m)]
    t, dtol = multi_maturity_tolerances(n_total or len(pts))
    law = (float(jump_intensity), float(jump_mean), float(jump_vol))
    launch = _bates_surface_launchers(solver, variant, r_d, r_f, m1, m2, theta, delta_t, snap_steps, grids, U_0, spots, scales,
                                      None if fit_jumps else law, dividends if variant == DIV else None, scheme=scheme)
    common = dict(dividends=dividends, max_iter=max_iter, tol=t if tol is None else tol,
                  delta_tol=dtol if delta_tol is None else delta_tol, scheme=scheme, launchers=launch)
    common.update(kw)
    if not fit_jumps:
        return calibrate(solver, variant, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0, market,
                         **common)
    res = calibrate(solver, variant, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0, market,
                    extra=law, clamp_extra=lambda lj, mj, sj: clamp_jump_parameters(lj, mj, sj, delta_t), solves_per_iteration=10,
                    **common)
    res["jump_intensity"], res["jump_mean"], res["jump_vol"] = res.pop("extra")
    return res


def calibrate_american_dividends_multi_maturity(solver, S_0, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, theta,
                                                calibration_points, grids, U_0, market_prices, dividends, max_iter=20,
                                                tol=0.1, **kw):
    return calibrate(solver, AM_DIV, S_0, None, r_d, r_f, kappa, eta, sigma, rho, V_0, m1, m2, None, theta, grids, U_0,
                     market_prices, dividends=dividends, calibration_points=calibration_points, max_iter=max_iter,
                     tol=tol, **kw)


def export_calibration_csv(path, result, S_0, r_d, strikes, market_prices, T=None, maturities=None, dividends=None,
                           elapsed_s=0.0, epsilon=0.01):
    """The drivers' result files (`fitted_heston_vs_market*.csv`): a '#' metadata line, then per instrument the
    market and fitted price with implied-vol difference (heston_calibration.cpp:443-511; multi-maturity layout
    with both implied vols :2851-2931; dividend drivers invert on the dividend-adjusted spot :1498-1530).
    `strikes` / `market_prices` cover ALL instruments in global order, `result["model_prices"]` likewise."""
    fitted = np.asarray(result["model_prices"], dtype=np.float64)
    market = np.asarray(market_prices, dtype=np.float64)
    k0, e0, s0, r0, v0 = result["initial"]
    tail = (", init_kappa=%g, init_eta=%g, init_sigma=%g, init_rho=%g, init_v0=%g, kappa=%g, eta=%g, sigma=%g, rho=%g, "
            "v0=%g\n" % (k0, e0, s0, r0, v0, result["kappa"], result["eta"], result["sigma"], result["rho"],
                          result["v0"]))

    def spot(T_):
        if dividends is None:
            return S_0
        S_adj = S_0
        for date, amount, pct in zip(dividends.dates, dividends.amounts, dividends.percentages):
            if date < T_:
                S_adj -= amount * math.exp(-r_d * date)
                S_adj -= (S_0 * pct) * math.exp(-r_d * date)
        return S_adj

    with open(path, "w") as out:
        if maturities is None:
            out.write("# %d options, Time=%g s, FinalError=%g, iterationCount=%d, TotalPdeSolves=%d" %
                      (len(strikes), elapsed_s, result["final_error"], result["iterations"], result["pde_solves"]) + tail)
            out.write("Strike,MarketPrice,FittedPrice,IVDifference\n")
            S = spot(T)
            for K, mp, fp in zip(strikes, market, fitted):
                d = abs(_market.reverse_BS(S, K, r_d, T, 0.5, mp, epsilon) - _market.reverse_BS(S, K, r_d, T, 0.5, fp, epsilon))
                out.write("%g,%g,%g,%g\n" % (K, mp, fp, d))
        else:
            out.write("# Calibration with %d maturities, %d strikes per maturity, Time=%g s, FinalError=%g, "
                      "IterationCount=%d, TotalPdeSolves=%d" % (len(maturities), len(strikes), elapsed_s,
                                                                result["final_error"], result["iterations"],
                                                                result["pde_solves"]) + tail)
            out.write("Maturity,Strike,MarketPrice,FittedPrice,MarketIV,FittedIV,IVDifference\n")
            for m, T_m in enumerate(maturities):
                S = spot(T_m)
                for s, K in enumerate(strikes):
                    idx = m * len(strikes) + s
                    miv = _market.reverse_BS(S, K, r_d, T_m, 0.5, market[idx], epsilon)
                    fiv = _market.reverse_BS(S, K, r_d, T_m, 0.5, fitted[idx], epsilon)
                    out.write("%g,%g,%g,%g,%g,%g,%g\n" % (T_m, K, market[idx], fitted[idx], miv, fiv, abs(miv - fiv)))


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _clone(x):
    return x.clone() if hasattr(x, "clone") else np.array(x, copy=True)
