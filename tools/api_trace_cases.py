#!/usr/bin/env python3
"""Diagnostic (needs a GPU): one call per driver and feature of csrc/hadi_api.hip, twice on a fresh handle (a capture and a replay
where the time loop is graphable), to be run under `rocprofv3 --kernel-trace --stats -- python tools/api_trace_cases.py CASE [--lib
OTHER_LIBHADI]` -- the per-kernel call counts of two builds must agree (profiles/api_refactor_trace.txt).  tools/api_refactor_ab.py
times the same calls.
    jac50          compute_jacobian, 50x25 x50 (300 instances), 20 steps
    jac_ladder     compute_jacobian_ladder, the same with snapshots behind steps 5, 10 and 20
    jac_samples    compute_jacobian_samples, 50x25 x8, 5 spots per instance, the same snapshots
    berm_stream    compute_base_prices_bermudan, 100x30 x16 on the streaming route (small_grid 0), a schedule per instance, 8 steps
    barrier        compute_base_prices_barrier, 50x25 x50, a double barrier monitored on 4 of 20 steps
    greeks_ladder  compute_greeks with the spot ladder, 50x25 x50, 20 steps"""
import os
import sys

import numpy as np

S_0, V_0, T, R_D, THETA = 100.0, 0.04, 1.0, 0.025, 0.8
MODEL = (-0.9, 0.3, 1.5, 0.04)  # rho sigma kappa eta
CASES = {"jac50": (50, 25, 50, 20), "jac_ladder": (50, 25, 50, 20), "jac_samples": (50, 25, 8, 20), "berm_stream": (100, 30, 16, 8),
         "barrier": (50, 25, 50, 20), "greeks_ladder": (50, 25, 50, 20)}


def prepare(H, sv, case):
    """Sets the handle up for `case` and returns the call as a function of nothing (host arrays, built once)."""
    m1, m2, n, N = CASES[case]
    strikes = [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    U0 = grids.call_payoff(strikes)
    m, dt = (m1 + 1) * (m2 + 1), T / N
    r_f = 0.0 if case in ("jac_ladder", "jac_samples") else 0.01
    mid = (R_D, r_f, *MODEL, m1, m2, m, N, THETA, dt, n, grids)
    ws = H.DOWorkspace(n, m)
    spots = np.array([[0.8 * k, 0.9 * k, k, 1.1 * k, 1.25 * k] for k in strikes])
    schedules = [[2 + k % 3, 6, 8][: 1 + k % 3] for k in range(n)]
    if case == "berm_stream":
        sv.set_tuning("small_grid", 0)

    def call():
        ws.U[...] = U0
        if case == "jac50":
            return sv.compute_jacobian(S_0, V_0, T, *mid, U0)
        if case == "jac_ladder":
            return sv.compute_jacobian_ladder(S_0, V_0, *mid, U0, [5, 10, 20])
        if case == "jac_samples":
            return sv.compute_jacobian_samples(spots, V_0, *mid, U0, [5, 10, 20])
        if case == "berm_stream":
            return sv.compute_base_prices_bermudan(S_0, V_0, *mid, ws, schedules)
        if case == "barrier":
            return sv.compute_base_prices_barrier(S_0, V_0, *mid, ws, [5, 10, 15, 20], lower=60.0, upper=160.0, rebate=1.0)
        return sv.compute_greeks(m1, m2, N, dt, THETA, R_D, r_f, *MODEL, grids, U0, S_0, V_0, ladder=True)

    return call


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import pde_based_heston_solver_gpu_accelerated_amd as H
    case = sys.argv[1]
    lib = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
    with H.HestonADI(0, lib_path=lib) as sv:
        call = prepare(H, sv, case)
        call()
        call()
        print(case, "|", sv.describe_last_sweep())


if __name__ == "__main__":
    main()
