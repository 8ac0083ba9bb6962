#!/usr/bin/env python3
"""Records tests/golden/route_selection_cliquet.json (needs a GPU): the description hadi_describe_last_sweep gives after a cliquet
call and after the plain call of the same batch, for the batches below -- every whole-loop kernel, the streaming kernels, a team-
and two resident-eligible batches, and the round plus remainder on two streams.  tests/test_emu_cliquet.py requires hadi_route and
hadi_describe_route to reproduce every row on the CPU; tests/test_gpu_cliquet.py requires the device to.
    python tools/record_cliquet_routes.py [--out FILE]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_selection_cliquet.json")
TH = {0: 0.8, 1: 0.5, 2: 1.0 / 3.0, 3: 0.7886751345948129}
# name, n, m1, m2, scheme, tuning, fixing steps (of N = 2), weights
CASES = [("block", 3, 50, 25, 0, {}, [1, 2], None), ("block weights", 3, 50, 25, 0, {}, [2], [0.5]),
         ("seq", 300, 50, 25, 0, {}, [1, 2], None), ("seq2", 600, 50, 25, 0, {}, [1], [1.0]),
         ("seq2 forced", 3, 50, 25, 0, {"small_seq": 1, "small_pairs": 1}, [1, 2], None), ("sch", 300, 50, 25, 2, {}, [1, 2], None),
         ("sch forced", 3, 50, 25, 2, {"small_sch": 1}, [2], [0.25]), ("streaming", 20, 300, 80, 0, {}, [1, 2], None),
         ("team-eligible", 4, 300, 140, 0, {}, [1, 2], [0.0, 1.0]), ("resident-eligible 300x80", 256, 300, 80, 0, {"resident_sweep": 1}, [1], None),
         ("resident-eligible 512x256", 256, 512, 256, 0, {}, [2], None), ("two streams", 320, 512, 256, 0, {}, [1, 2], None)]
DEFAULTS = {"small_seq": -1, "small_pairs": -1, "small_sch": -1, "resident_sweep": -1}


def describe(sv, H, np, case):
    """(the plain call's description, the cliquet call's)."""
    name, n, m1, m2, scheme, tuning, steps, weights = case
    strikes = [85.0 + 30.0 * k / max(n - 1, 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, 100.0, 0.04, strikes)
    ref = np.array([g.Vec_s[k][int(np.argmin(np.abs(g.Vec_s[k] - strikes[k])))] for k in range(n)])
    head = (m1, m2, 2, 0.5, TH[scheme], 0.025, 0.0, -0.9, 0.3, 1.5, 0.04, g)
    for k, v in tuning.items():
        sv.set_tuning(k, v)
    try:
        sv.DO_timestepping(*head, g.call_payoff(strikes), scheme=scheme)
        d0 = sv.describe_last_sweep()
        sv.cliquet_timestepping(*head, g.call_payoff(strikes), steps, ref, H.FIX_SHARES, weights, scheme=scheme)
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
                         "fix_steps": case[6], "weights": case[7], "plain": d0, "cliquet": d1})
            print(case[0], "|", d1)
    with open(out, "w") as f:
        json.dump({"cu_count": cus, "cases": rows}, f, indent=1)
        f.write("\n")
