"""tests/golden/kernel_selection.json against the library itself: one small batch per row-pass and column-pass family on the
streaming path.  hadi_describe_last_sweep must begin with the fixture's description for the same inputs (the CPU test
tests/test_kernel_selection.py ties that text to the selected kernels), and the field must match the oracle."""
import json
import os

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm

pytestmark = pytest.mark.gpu

FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_selection.json")))
R_F = 0.01  # (the strip kernels need r_d != r_f)
N_INST, N_STEPS = 4, 2
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "pair_strips": -1}

#        name                 m1   m2   tuning                           scheme
CASES = [("ring",             50,  25,  {},                              H.SCHEME_DOUGLAS),
         ("strips_b2",        100, 50,  {"strip": 1},                    H.SCHEME_DOUGLAS),
         ("strips_b4",        200, 60,  {"strip": 1},                    H.SCHEME_DOUGLAS),
         ("strips_b8",        300, 80,  {"strip": 1},                    H.SCHEME_DOUGLAS),
         ("paired_strips",    600, 40,  {"strip": 1},                    H.SCHEME_DOUGLAS),
         ("pairs",            200, 60,  {"strip": 1, "pair_strips": 1},  H.SCHEME_DOUGLAS),
         ("row_seq",          1100, 20, {},                              H.SCHEME_DOUGLAS),
         ("chunks_9_to_16",   50,  300, {},                              H.SCHEME_DOUGLAS),
         ("col_seq",          40,  600, {},                              H.SCHEME_DOUGLAS),
         ("craig_sneyd_strips", 300, 80, {"strip": 1},                   H.SCHEME_CRAIG_SNEYD)]


def _fixture_description(m1, m2, tune, scheme):
    want = [m1, m2, N_INST, tune.get("strip", -1), tune.get("pair_strips", -1), 0, 0, 0, 0, 0, int(scheme), 1, 0]
    hits = [c for c in FIX["cases"] if c["in"] == want]
    assert len(hits) == 1, want
    return hits[0]["desc"]


@pytest.mark.parametrize("name,m1,m2,tune,scheme", CASES, ids=[c[0] for c in CASES])
def test_family_on_the_streaming_path(solver, name, m1, m2, tune, scheme):
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the fixture records the plans of the 256-CU device")
    want = _fixture_description(m1, m2, tune, scheme)
    strikes = Cm.well_conditioned_strikes(m1, N_INST)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0_ALT, strikes)  # (V_0 = 0.04 breaks the 30x rule at m2 = 300)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(strikes)
    U = U0.copy()
    for k, v in {**STREAMING, **tune}.items():
        solver.set_tuning(k, v)
    try:
        solver.DO_timestepping(m1, m2, N_STEPS, Cm.T / N_STEPS, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               scheme=scheme)
        d = solver.describe_last_sweep()
    finally:
        for k, v in DEFAULTS.items():
            solver.set_tuning(k, v)
    assert d.startswith(want), (d, want)
    p = O.make_params(m1, m2, N_STEPS, Cm.T / N_STEPS, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
    p.scheme = 1 if scheme == H.SCHEME_CRAIG_SNEYD else 0
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)
    err = np.abs(U - Uo).max() / np.abs(Uo).max()
    print("%s: field error %.3e" % (name, err))
    assert err <= 1e-10, err
