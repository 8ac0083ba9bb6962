#!/usr/bin/env python3
"""Diagnostic (needs a GPU): the strike surface from one sweep against the ladder launchers, the non-sample calls against a build
of the commit before, and the cost of hadi_sample_kernel.
    python tools/surface_ab.py [--lib PARENT_LIB] [--rounds R]
1. Non-sample calls, this build against PARENT_LIB (skipped without --lib), alternating: the bench.py headline shape (512x256, 256
   European calls, hadi_DO_timestepping; 100 of its 1000 steps), the harness shape 50x25x20 with 1 and 500 options
   (compute_base_prices) and 50x25 x 40 steps x 3000 options (hadi_DO_timestepping).  The parent's spread (max - min over its rounds)
   is the margin.
2. Surface against the ladder launchers of this build.  Surfaces of 50 and 500 strikes (85 .. 115) x 10 evenly spaced maturities
   (n_k = 10 .. 100 steps of 0.05): the ladder runs one 50x25 instance per strike (compute_jacobian_ladder /
   compute_base_prices_ladder), the surface ONE instance built at K = 100 on 50x25, 100x50 and 200x100
   (compute_jacobian_samples / compute_base_prices_samples through strike_samples).  ms per call and, beside them, the largest
   difference of the surface's prices from the per-strike ladder's -- a difference of discretisations (scaled grid against the
   grid built per strike), to be read against the grids' own error.
3. hadi_sample_kernel: 512x256 x 256 instances x 64 samples, 20 steps, a snapshot behind every step against a snapshot behind the
   last step only: the difference over 19 is the cost per snapshot launch, beside the time of a step.
Wall-clock ms per call (every call ends with a stream synchronisation), one warm-up round, then R rounds alternating; min, median,
spread.  Device-resident inputs throughout."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

LIB, ROUNDS = None, 7
if "--lib" in sys.argv:
    k = sys.argv.index("--lib")
    LIB = sys.argv[k + 1]
    del sys.argv[k:k + 2]
if "--rounds" in sys.argv:
    k = sys.argv.index("--rounds")
    ROUNDS = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
S_0, V_0, R_D, R_F = 100.0, 0.04, 0.025, 0.0
MODEL = (-0.9, 0.3, 1.5, 0.04)  # rho, sigma, kappa, eta
THETA = 0.8
DEV = torch.device("cuda:0")


class WS:
    pass


def ws(u):
    w = WS()
    w.U = u.clone()
    return w


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return "min %8.3f  median %8.3f  spread %7.3f" % (min(t), statistics.median(t), max(t) - min(t))


def strikes_for(n):
    return [100.0] if n == 1 else [85.0 + 30.0 * k / (n - 1) for k in range(n)]


def batch(m1, m2, strikes):
    g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    return g.to(DEV), torch.from_numpy(g.call_payoff(strikes)).to(DEV)


def non_sample_ab(new, old):
    rho, sigma, kappa, eta = MODEL
    jobs = []
    g, u = batch(512, 256, strikes_for(256))
    jobs.append(("512x256 x256 x100 steps DO_timestepping", 1,
                 lambda sv, g=g, u=u: sv.DO_timestepping(512, 256, 100, 0.001, THETA, R_D, R_F, rho, sigma, kappa, eta, g, u.clone())))
    for n in (1, 500):
        g, u = batch(50, 25, strikes_for(n))
        jobs.append(("50x25x20 x%d EU base prices" % n, 20,
                     lambda sv, n=n, g=g, u=u: sv.compute_base_prices(S_0, V_0, 1.0, R_D, R_F, rho, sigma, kappa, eta, 50, 25, 51 * 26, 20,
                                                                      THETA, 0.05, n, g, ws(u))))
    g, u = batch(50, 25, strikes_for(3000))
    jobs.append(("50x25 x3000 x40 steps DO_timestepping", 3,
                 lambda sv, g=g, u=u: sv.DO_timestepping(50, 25, 40, 0.025, THETA, R_D, R_F, rho, sigma, kappa, eta, g, u.clone())))
    print("## 1. non-sample calls: this build against the build of the commit before, ms per call, alternating")
    for name, reps, fn in jobs:
        tn, to = [], []
        for rnd in range(ROUNDS + 1):
            a, _ = timed(lambda: [fn(old) for _ in range(reps)])
            path_o = old.describe_last_sweep()
            b, _ = timed(lambda: [fn(new) for _ in range(reps)])
            path_n = new.describe_last_sweep()
            if rnd:
                to.append(a / reps)
                tn.append(b / reps)
        spread = max(to) - min(to)
        diff = statistics.median(tn) - statistics.median(to)
        print("%-42s parent %s | %s" % (name, stats(to), path_o[:50]))
        print("%-42s new    %s | %s" % (name, stats(tn), path_n[:50]))
        print("# %s: new - parent = %+.4f ms (medians), the parent's spread %.4f ms: %s" % (
            name, diff, spread, "within the margin" if diff <= spread else "SLOWER THAN THE MARGIN"), flush=True)


def surface_vs_ladder(sv, n_s, steps, dt):
    rho, sigma, kappa, eta = MODEL
    strikes = strikes_for(n_s)
    N = steps[-1]
    gl, ul = batch(50, 25, strikes)
    spots, scales = H.strike_samples(S_0, 100.0, strikes)
    calls = [("ladder 50x25 x%d" % n_s,
              lambda: sv.compute_jacobian_ladder(S_0, V_0, R_D, R_F, rho, sigma, kappa, eta, 50, 25, 51 * 26, N, THETA, dt, n_s, gl, ul, steps),
              lambda: sv.compute_base_prices_ladder(S_0, V_0, R_D, R_F, rho, sigma, kappa, eta, 50, 25, 51 * 26, N, THETA, dt, n_s, gl, ws(ul),
                                                    steps))]
    for m1, m2 in ((50, 25), (100, 50), (200, 100)):
        g, u = batch(m1, m2, [100.0])
        tot = (m1 + 1) * (m2 + 1)
        calls.append(("surface %dx%d x1" % (m1, m2),
                      lambda g=g, u=u, m1=m1, m2=m2, tot=tot: sv.compute_jacobian_samples(spots, V_0, R_D, R_F, rho, sigma, kappa, eta, m1, m2, tot, N,
                                                                                        THETA, dt, 1, g, u, steps, scales=scales),
                      lambda g=g, u=u, m1=m1, m2=m2, tot=tot: sv.compute_base_prices_samples(spots, V_0, R_D, R_F, rho, sigma, kappa, eta, m1, m2, tot,
                                                                                           N, THETA, dt, 1, g, ws(u), steps, scales=scales)))
    print("## 2. %d strikes x %d maturities (n_k = %s, delta_t = %g)" % (n_s, len(steps), steps, dt))
    tj, tb = {c[0]: [] for c in calls}, {c[0]: [] for c in calls}
    prices, paths = {}, {}
    for rnd in range(ROUNDS + 1):  # (round 0 warms everything up and is not counted)
        for name, jac, base in calls:
            a, _ = timed(jac)
            b, p = timed(base)
            paths[name] = sv.describe_last_sweep()
            prices[name] = p.cpu().numpy()
            if rnd:
                tj[name].append(a)
                tb[name].append(b)
    lad = prices[calls[0][0]].T  # [s][m] -> [m][s]
    for name, _, _ in calls:
        diff = "" if name.startswith("ladder") else "  prices vs the per-strike ladder: max |diff| %.3e" % np.abs(prices[name][0] - lad).max()
        print("%-20s Jacobian    %s" % (name, stats(tj[name])))
        print("%-20s base prices %s%s | %s" % (name, stats(tb[name]), diff, paths[name][:60]), flush=True)
    for name, _, _ in calls[1:]:
        print("# %s: ladder / surface = %.2fx Jacobian, %.2fx base prices (medians)" % (
            name, statistics.median(tj[calls[0][0]]) / statistics.median(tj[name]), statistics.median(tb[calls[0][0]]) / statistics.median(tb[name])))


def sample_kernel_cost(sv):
    rho, sigma, kappa, eta = MODEL
    m1, m2, n, N, n_samp = 512, 256, 256, 20, 64
    g, u = batch(m1, m2, strikes_for(n))
    spots = np.linspace(81.3, 119.7, n_samp)
    run = lambda snaps: sv.sample_ladder(m1, m2, N, 0.001, THETA, R_D, R_F, rho, sigma, kappa, eta, g, u, spots, V_0, snaps)
    every, last = list(range(1, N + 1)), [N]
    te, tl = [], []
    for rnd in range(ROUNDS + 1):
        a, _ = timed(lambda: run(every))
        path = sv.describe_last_sweep()
        b, _ = timed(lambda: run(last))
        if rnd:
            te.append(a)
            tl.append(b)
    per = (statistics.median(te) - statistics.median(tl)) / (N - 1)
    print("## 3. hadi_sample_kernel: %dx%d x %d instances x %d samples, %d steps" % (m1, m2, n, n_samp, N))
    print("a snapshot behind every step %s | %s" % (stats(te), path[-90:]))
    print("a snapshot behind the last   %s" % stats(tl))
    print("# per snapshot launch: %.1f us beside %.1f us per step (whole call / %d, staging included): %.2f %% of a step" % (
        per * 1e3, statistics.median(tl) / N * 1e3, N, 100.0 * per / (statistics.median(tl) / N)), flush=True)


sv = H.HestonADI(0)
print("# device: %s" % sv.device_info())
if LIB:
    old = H.HestonADI(0, lib_path=LIB)
    non_sample_ab(sv, old)
    old.close()
else:
    print("## 1. non-sample calls: no --lib PARENT_LIB given, not measured")
ten = [10 * k for k in range(1, 11)]
surface_vs_ladder(sv, 50, ten, 0.05)
surface_vs_ladder(sv, 500, ten, 0.05)
sample_kernel_cost(sv)
sv.close()
