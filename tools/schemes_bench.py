#!/usr/bin/env python3
"""Diagnostic (needs a GPU): ms per time step of the four splitting schemes -- Douglas, Craig-Sneyd, Modified Craig-Sneyd
(theta = 1/3), Hundsdorfer-Verwer (theta = 1/2 + sqrt(3)/6) -- on 512x256 x256, 1024x512 x64 and 50x25 x500 (or one shape).
    python tools/schemes_bench.py [instances steps m1 m2]
Device-resident inputs, sweep-only events (hadi_timing.sweep_ms), best of three; the kernels each scheme ran."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

SHAPES = [(256, 100, 512, 256), (64, 100, 1024, 512), (500, 100, 50, 25)]
if len(sys.argv) > 4:
    SHAPES = [tuple(int(a) for a in sys.argv[1:5])]
SCHEMES = [("Douglas", H.SCHEME_DOUGLAS, 0.8), ("Craig-Sneyd", H.SCHEME_CRAIG_SNEYD, 0.8),
           ("MCS", H.SCHEME_MCS, 1.0 / 3.0), ("HV", H.SCHEME_HV, 0.5 + math.sqrt(3.0) / 6.0)]
dev = torch.device("cuda:0")
s = H.HestonADI(0)
for n, N, m1, m2 in SHAPES:
    ks = [85.0 + 30.0 * k / max(1, n - 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, 100.0, 0.04, ks)
    u0 = torch.from_numpy(g.call_payoff(ks)).to(dev)
    gd = g.to(dev)
    base = None
    for name, scheme, theta in SCHEMES:
        best = 1e30
        for rep in range(3):
            u = u0.clone()
            torch.cuda.synchronize()
            s.DO_timestepping(m1, m2, N, 1.0 / 1000, theta, 0.025, 0.0, -0.9, 0.3, 1.5, 0.04, gd, u, scheme=scheme)
            torch.cuda.synchronize()
            best = min(best, s.timing()["sweep_ms"])
        if scheme == H.SCHEME_CRAIG_SNEYD:
            base = best
        rel = "" if base is None or scheme < H.SCHEME_CRAIG_SNEYD else "  %+.1f %% vs CS" % (100.0 * (best / base - 1.0))
        print("%dx%d x%d %-12s %.4f ms per step%s | %s" % (m1, m2, n, name, best / N, rel, s.describe_last_sweep()), flush=True)
s.close()
