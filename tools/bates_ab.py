#!/usr/bin/env python3
"""Diagnostic (needs a GPU): what the Bates entry points cost, and that the plain calls cost what they did.
    python tools/bates_ab.py [--parent PARENT_TREE] [--rounds R] [--out FILE]
(1) Plain calls, this tree against PARENT_TREE (a built checkout of the commit before; skipped without --parent): hadi_DO_timestepping
    on 50x25 x 3000 and on 512x256 x 256, both libraries loaded into this process, R alternating rounds (default 7), wall ms per call
    (best of 3 in every round).  The allowance is the spread (max - min) of the parent's own rounds; a difference of the means
    beyond it is flagged.
(2) The jump sub-step beside a plain step, on the streaming kernels (small_grid, team_launch and resident_sweep pinned to 0 for the
    plain call; a jump call takes them anyway) at 50x25 x 500, 256x128 x 64 and 512x256 x 256, the last both with one shared matrix
    (every instance on one s-grid) and with per-instance matrices.  Under hadi_set_profiling the sub-step's time -- the copy of U
    to U_temp and hadi_jump_kernel -- is the difference of the sweeps over the steps, set against the same run's two passes per
    step; the achieved fp64 rate is 2 (m1 + 1)^2 (m2 + 1) flop per instance and step over that time, as a fraction of 78.6 TFLOP/s,
    the MI355X data sheet's fp64 matrix peak.  The cost of the per-call matrix build is the difference of the two calls' set-up
    times (hadi_timing.setup_ms: staging, hadi_jump_matrix_kernel, the shared-grid check).
The text goes to stdout and to FILE (default profiles/bates_ab.txt)."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def opt(name, default, conv=str):
    if name in sys.argv:
        k = sys.argv.index(name)
        v = conv(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        return v
    return default


PARENT, ROUNDS = opt("--parent", None), opt("--rounds", 7, int)
OUT = opt("--out", os.path.join(ROOT, "profiles", "bates_ab.txt"))
LINES = []

import numpy as np
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

DEV = torch.device("cuda:0")
S_0, V_0, T, R_D, R_F, THETA = 100.0, 0.04, 1.0, 0.025, 0.0, 0.8
MODEL = (-0.9, 0.3, 1.5, 0.04)
JUMPS = (0.5, -0.10, 0.15)
PEAK_FP64_MATRIX = 78.6e12  # MI355X data sheet, fp64 matrix
STREAMING, DEFAULT = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}, {"small_grid": 1, "team_launch": -1, "resident_sweep": -1}


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=3):
    best = 1e30
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def problem(m1, m2, n, same=False):
    strikes = [100.0] * n if same else [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    return strikes, g, g.to(DEV), torch.from_numpy(g.call_payoff(strikes)).to(DEV)


def part_1(sv):
    say("## (1) plain hadi_DO_timestepping, this tree against the parent commit's, %d alternating rounds, wall ms per call (best of 3 per round)" % ROUNDS)
    old = H.HestonADI(0, lib_path=os.path.join(PARENT, "pde_based_heston_solver_gpu_accelerated_amd", "libhadi.so"))
    for m1, m2, N, n in ((50, 25, 50, 3000), (512, 256, 20, 256)):
        strikes, g, gd, u0 = problem(m1, m2, n)
        u = torch.empty_like(u0)

        def call(s):
            u.copy_(u0)
            s.DO_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u)

        call(old), call(sv)
        d_old, d_new = old.describe_last_sweep(), sv.describe_last_sweep()
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(timed(lambda: call(old)))
            b.append(timed(lambda: call(sv)))
        ma, mb, sa, sb = statistics.mean(a), statistics.mean(b), max(a) - min(a), max(b) - min(b)
        verdict = "within the parent's own spread" if abs(mb - ma) <= sa else ("SLOWER BEYOND THE SPREAD" if mb > ma else "faster beyond the spread")
        say("%dx%d x %d steps x %d: parent mean %.4f spread %.4f | new mean %.4f spread %.4f | new - parent %+.4f ms (%+.2f %%): %s" % (
            m1, m2, N, n, ma, sa, mb, sb, mb - ma, 100.0 * (mb - ma) / ma, verdict))
        say("    parent rounds %s" % " ".join("%.4f" % x for x in a))
        say("    new rounds    %s" % " ".join("%.4f" % x for x in b))
        say("    route: %s%s" % (d_new[:160], "" if d_new == d_old else "  [PARENT: %s]" % d_old[:160]))
    old.close()


def part_2(sv):
    say("## (2) the jump sub-step on every step against none, streaming kernels, calls, device-resident inputs, lambda %g mu_J %g sigma_J %g" % JUMPS)
    for key, val in STREAMING.items():
        sv.set_tuning(key, val)
    N = 20
    for m1, m2, n, same in ((50, 25, 500, False), (256, 128, 64, False), (512, 256, 256, True), (512, 256, 256, False)):
        strikes, g, gd, u0 = problem(m1, m2, n, same)
        u = torch.empty_like(u0)
        flop = 2.0 * (m1 + 1) ** 2 * (m2 + 1) * n

        def plain():
            u.copy_(u0)
            sv.DO_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u)

        def bates():
            u.copy_(u0)
            sv.bates_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u, *JUMPS, shared_grid=same)

        runs = (("plain", plain), ("bates", bates))
        wall, prof = {}, {}
        for name, fn in runs:
            fn()
            wall[name] = timed(fn)
        d = sv.describe_last_sweep()
        sv.set_profiling(1)
        for name, fn in runs:
            fn()
            rs = []
            for _ in range(3):
                fn()
                rs.append(sv.timing())
            prof[name] = (min(rs, key=lambda t: t["sweep_ms"]), min(t["setup_ms"] for t in rs))
        sv.set_profiling(0)
        p, b = prof["plain"][0], prof["bates"][0]
        row, col = p["pass_a_ms"] / max(1, p["pass_a_launches"]), p["pass_b_ms"] / max(1, p["pass_b_launches"])
        per = (b["sweep_ms"] - p["sweep_ms"]) / N
        rate = flop / (per * 1e-3) if per > 0 else float("nan")
        say("%dx%d x %d steps x %d, %s: plain %.3f ms, Bates %.3f ms per call (%+.1f %%)" % (
            m1, m2, N, n, "ONE shared matrix" if same else "per-instance matrices", wall["plain"], wall["bates"],
            100.0 * (wall["bates"] / wall["plain"] - 1.0)))
        say("    %s" % d[:300])
        say("    under profiling: copy + hadi_jump_kernel %.4f ms per step beside row pass %.4f + column pass %.4f ms per step (%.2fx a "
            "step's two passes); %.2f TFLOP/s fp64 = %.3f of the %.1f TFLOP/s fp64 matrix peak" % (
                per, row, col, per / (row + col), rate / 1e12, rate / PEAK_FP64_MATRIX, PEAK_FP64_MATRIX / 1e12))
        say("    matrix build per call (difference of the set-up times): %.4f ms (set-up plain %.4f, Bates %.4f); %.1f MB of matrix entries" % (
            prof["bates"][1] - prof["plain"][1], prof["plain"][1], prof["bates"][1], (1 if same else n) * 8.0 * (m1 + 1) ** 2 / 1e6))
    for key, val in DEFAULT.items():
        sv.set_tuning(key, val)


sv = H.HestonADI(0)
say("device %s" % sv.device_info())
if PARENT:
    part_1(sv)
else:
    say("## (1) plain calls: no --parent PARENT_TREE given, not measured")
part_2(sv)
sv.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
