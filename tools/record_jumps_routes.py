#!/usr/bin/env python3
"""Records tests/golden/route_selection_jumps.json (needs a GPU): the description hadi_describe_last_sweep gives after a Bates
call and after the plain call of the same batch, for the batches below -- every batch that would take a whole-loop kernel, the
streaming kernels, a team- and two resident-eligible batches, and the round plus remainder on two streams.  A jump call takes the
streaming path on all of them.  tests/test_emu_jumps.py requires hadi_route and hadi_describe_route to reproduce every row on the
CPU; tests/test_gpu_jumps.py requires the device to.
    python tools/record_jumps_routes.py [--out FILE]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_selection_jumps.json")
TH = {0: 0.8, 1: 0.5, 2: 1.0 / 3.0, 3: 0.7886751345948129}
JUMPS = (0.5, -0.10, 0.15)  # lambda, mu_J, sigma_J
# name, n, m1, m2, scheme, tuning
CASES = [("block", 3, 50, 25, 0, {}), ("seq", 300, 50, 25, 0, {}), ("seq2", 600, 50, 25, 0, {}),
         ("seq2 forced", 3, 50, 25, 0, {"small_seq": 1, "small_pairs": 1}), ("sch", 300, 50, 25, 2, {}),
         ("sch forced", 3, 50, 25, 2, {"small_sch": 1}), ("streaming", 20, 300, 80, 0, {}), ("streaming HV", 5, 100, 50, 3, {}),
         ("team-eligible", 4, 300, 140, 0, {}), ("resident-eligible 300x80", 256, 300, 80, 0, {"resident_sweep": 1}),
         ("resident-eligible 512x256", 256, 512, 256, 0, {}), ("two streams", 320, 512, 256, 0, {})]
DEFAULTS = {"small_seq": -1, "small_pairs": -1, "small_sch": -1, "resident_sweep": -1}


def describe(sv, H, np, case):
    """(the plain call's description, the Bates call's)."""
    name, n, m1, m2, scheme, tuning = case
    strikes = [85.0 + 30.0 * k / max(n - 1, 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, 100.0, 0.04, strikes)
    head = (m1, m2, 2, 0.5, TH[scheme], 0.025, 0.0, -0.9, 0.3, 1.5, 0.04, g)
    for k, v in tuning.items():
        sv.set_tuning(k, v)
    try:
        sv.DO_timestepping(*head, g.call_payoff(strikes), scheme=scheme)
        d0 = sv.describe_last_sweep()
        sv.bates_timestepping(*head, g.call_payoff(strikes), *JUMPS, scheme=scheme)
        return d0, sv.describe_last_sweep()
    finally:
        for k in tuning:
            sv.set_tuning(k, DEFAULTS[k])


if __name__ == "__main__":
    import numpy as np
    import pde_based_heston_solver_gpu_accelerated_amd as H
    out = FIXTURE if "--out" not in sys.argv else sys.argv[sys.argv.index("--out") + 1]
    with H.HestonADI(0) as sv:
        cus = sv.device_info()["compute_units"]
        rows = []
        for case in CASES:
            d0, d1 = describe(sv, H, np, case)
            rows.append({"name": case[0], "n": case[1], "m1": case[2], "m2": case[3], "scheme": case[4], "tuning": case[5],
                         "plain": d0, "bates": d1})
            print(case[0], "|", d1)
    with open(out, "w") as f:
        json.dump({"cu_count": cus, "cases": rows}, f, indent=1)
        f.write("\n")
