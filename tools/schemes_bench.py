#!/usr/bin/env python3
"""Diagnostic (needs a GPU): ms per time step of the four splitting schemes -- Douglas, Craig-Sneyd, Modified Craig-Sneyd
(theta = 1/3), Hundsdorfer-Verwer (theta = 1/2 + sqrt(3)/6) -- on 512x256 x256, 1024x512 x64 and 50x25 x500 (or one shape).
    python tools/schemes_bench.py [--lib PATH] [instances steps m1 m2]
Device-resident inputs, sweep-only events (hadi_timing.sweep_ms), best of three; the kernels each scheme ran.  --lib PATH loads
another build of libhadi.so (e.g. one of the commit before) instead of the tree's.
    python tools/schemes_bench.py --small-sch-ab [--lib PARENT_LIB]
A/B of the LDS-resident predictor-corrector kernel (tuning key "small_sch"): MCS and HV on 50x25 x257 / x500 / x1024 / x3000 and
100x30 x500, N = 100, five rounds of (PARENT_LIB if given, this build with "small_sch" = 1, this build with "small_sch" = 0) in
that order in one process; what the automatic rule ("small_sch" = -1) picks for the batch, min, median and spread (max - min) of the sweep time per step of each side, the gain criterion of
DESIGN.md section 4.1 (median gain > 2 x the parent's spread), and the two paths' fields against each other at 50x25 x3000."""
import math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import numpy as np
import pde_based_heston_solver_gpu_accelerated_amd as H

LIB = None
if "--lib" in sys.argv:
    k = sys.argv.index("--lib")
    LIB = sys.argv[k + 1]
    del sys.argv[k:k + 2]
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0


def well_conditioned_batch(m1, m2, n):
    """The first n of the strikes 85 + 30 k / 4095 whose s-grid keeps neighbouring intervals within 30x."""
    cand = [85.0 + 30.0 * k / 4095 for k in range(4096)]
    ds = H.GridViewsBatch.for_strikes(m1, 8, 100.0, 0.04, cand).Delta_s
    ok = np.maximum(ds[:, 1:] / ds[:, :-1], ds[:, :-1] / ds[:, 1:]).max(axis=1) <= 30.0
    ks = [c for c, good in zip(cand, ok) if good][:n]
    assert len(ks) == n
    g = H.GridViewsBatch.for_strikes(m1, m2, 100.0, 0.04, ks)
    return g, g.call_payoff(ks)


def small_sch_ab():
    dev = torch.device("cuda:0")
    sides = []
    if LIB:
        sides.append(("parent", H.HestonADI(0, lib_path=LIB), None))
    sides += [("new", H.HestonADI(0), 1), ("new, small_sch=0", H.HestonADI(0), 0)]
    for name, sv, key in sides:
        if key is not None:
            sv.set_tuning("small_sch", key)
    N = 100
    for n, m1, m2 in [(257, 50, 25), (500, 50, 25), (1024, 50, 25), (3000, 50, 25), (500, 100, 30)]:
        g, U0 = well_conditioned_batch(m1, m2, n)
        u0, gd = torch.from_numpy(U0).to(dev), g.to(dev)
        for sname, scheme, theta in (("MCS", H.SCHEME_MCS, TH_MCS), ("HV", H.SCHEME_HV, TH_HV)):
            times = {name: [] for name, _, _ in sides}
            fields, paths = {}, {}
            for rnd in range(6):  # (round 0 warms every side up and is not counted)
                for name, sv, _ in sides:
                    u = u0.clone()
                    torch.cuda.synchronize()
                    sv.DO_timestepping(m1, m2, N, 1.0 / N, theta, 0.025, 0.007, -0.9, 0.3, 1.5, 0.04, gd, u, scheme=scheme)
                    torch.cuda.synchronize()
                    if rnd:
                        times[name].append(sv.timing()["sweep_ms"] / N)
                    else:
                        fields[name], paths[name] = u.cpu().numpy(), sv.describe_last_sweep()
            auto = sides[-1][1]  # (what the automatic rule picks: one step on the handle whose key goes back to 0 afterwards)
            auto.set_tuning("small_sch", -1)
            auto.DO_timestepping(m1, m2, 1, 1.0 / N, theta, 0.025, 0.007, -0.9, 0.3, 1.5, 0.04, gd, u0.clone(), scheme=scheme)
            picked = auto.describe_last_sweep()
            auto.set_tuning("small_sch", 0)
            print("# %dx%d x%d %s, N = %d, ms per step; the automatic rule picks %s" % (
                m1, m2, n, sname, N, "the new kernel" if "hadi_small_sch_kernel" in picked else "the streaming kernels"))
            for name, _, _ in sides:
                t = times[name]
                print("%-17s min %.5f  median %.5f  spread %.5f  runs %s | %s" % (name, min(t), statistics.median(t), max(t) - min(t),
                                                                                 " ".join("%.5f" % x for x in t), paths[name].split(":")[0][:60]))
            if LIB:
                tp, tn = times["parent"], times["new"]
                gain, spread = statistics.median(tp) - statistics.median(tn), max(tp) - min(tp)
                print("# new against parent: %.2fx (median), gain %.5f ms = %.1f x the parent's spread, every new run faster than every "
                      "parent run: %s -> criterion %s" % (statistics.median(tp) / statistics.median(tn), gain, gain / spread if spread else float("inf"),
                                                          max(tn) < min(tp), "MET" if gain > 2 * spread and max(tn) < min(tp) else "NOT MET"))
            a, b = fields["new"], fields["new, small_sch=0"]
            rel = float(np.abs(a - b).max() / np.abs(b).max())
            print("# fields, new path against small_sch=0: max|dU| / max|U| = %.2e (bound 1e-11 N / 4 = %.1e): %s" % (
                rel, 1e-11 * N / 4, "ok" if rel <= 1e-11 * N / 4 else "TOO LARGE"), flush=True)
    for _, sv, _ in sides:
        sv.close()


if "--small-sch-ab" in sys.argv:
    small_sch_ab()
    sys.exit(0)

SHAPES = [(256, 100, 512, 256), (64, 100, 1024, 512), (500, 100, 50, 25)]
if len(sys.argv) > 4:
    SHAPES = [tuple(int(a) for a in sys.argv[1:5])]
SCHEMES = [("Douglas", H.SCHEME_DOUGLAS, 0.8), ("Craig-Sneyd", H.SCHEME_CRAIG_SNEYD, 0.8),
           ("MCS", H.SCHEME_MCS, 1.0 / 3.0), ("HV", H.SCHEME_HV, 0.5 + math.sqrt(3.0) / 6.0)]
dev = torch.device("cuda:0")
s = H.HestonADI(0, lib_path=LIB) if LIB else H.HestonADI(0)
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
        print("%dx%d x%d %-12s %.6f ms per step%s | %s" % (m1, m2, n, name, best / N, rel, s.describe_last_sweep()), flush=True)
s.close()
