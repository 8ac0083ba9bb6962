#!/usr/bin/env python3
"""Diagnostic (needs a GPU): what the eight-column Bates Jacobian costs, and that the existing calls cost what they did.
    python tools/bates_jacobian_ab.py [--parent PARENT_TREE] [--rounds R] [--out FILE]
(a) Existing calls, this tree against PARENT_TREE (a built checkout of the commit before; skipped without --parent): plain
    hadi_DO_timestepping and hadi_compute_jacobian_bates on 50x25 x 3000 and on 512x256 x 256, both libraries loaded into this
    process, R alternating rounds (default 5), wall ms per call (best of 3 in every round).  The allowance is the spread (max - min)
    of the parent's own rounds; a difference of the means beyond it is flagged.
(b) hadi_compute_jacobian_bates_jumps (nine groups, three matrix sets) beside hadi_compute_jacobian_bates (six groups, one set) at
    50x25 x 500 x 20 steps and 256x128 x 64 x 20 steps, per-instance matrices, alternating rounds; the matrix build split out as the
    set-up time under hadi_set_profiling (staging, v-grid rebuild, hadi_jump_matrix_kernel).
(c) The same eight-column call with "jump_share" 1 (the groups 0 .. 6 of an instance on one staged strip of G) and 0 (one instance
    per block), alternating rounds: the rule is to ship sharing only if it is faster beyond the run-to-run spread at 50x25 x 500.
(d) One LM iteration of calibrate_bates_jumps (one eight-column Jacobian, the 73 partial sums on the device, one trial) on 500
    strikes of 50x25, 20 steps, device-resident inputs, beside one iteration of calibrate_bates and of calibrate_european.
The text goes to stdout and to FILE (default profiles/bates_jacobian_ab.txt)."""
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


PARENT, ROUNDS = opt("--parent", None), opt("--rounds", 5, int)
OUT = opt("--out", os.path.join(ROOT, "profiles", "bates_jacobian_ab.txt"))
LINES = []

import numpy as np
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

DEV = torch.device("cuda:0")
S_0, V_0, T, R_D, R_F, THETA = 100.0, 0.04, 1.0, 0.025, 0.0, 0.8
MODEL = (-0.9, 0.3, 1.5, 0.04)
JUMPS = (0.5, -0.10, 0.15)


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


def problem(m1, m2, n):
    strikes = [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    return strikes, g, g.to(DEV), torch.from_numpy(g.call_payoff(strikes)).to(DEV)


def alternate(fa, fb, rounds=None):
    """R alternating rounds of two calls: (means, spreads, rounds)."""
    fa(), fb()
    a, b = [], []
    for _ in range(rounds or ROUNDS):
        a.append(timed(fa))
        b.append(timed(fb))
    return (statistics.mean(a), statistics.mean(b)), (max(a) - min(a), max(b) - min(b)), (a, b)


def verdict(ma, mb, sa):
    return "within the first one's own spread" if abs(mb - ma) <= sa else ("SLOWER BEYOND THE SPREAD" if mb > ma else "faster beyond the spread")


def jac_args(m1, m2, N, n, gd, u0):
    return (S_0, V_0, R_D, R_F) + MODEL + (m1, m2, (m1 + 1) * (m2 + 1), N, THETA, T / N, n, gd, u0) + JUMPS


def part_a(sv):
    say("## (a) existing calls, the parent commit's library against this tree's, %d alternating rounds, wall ms per call (best of 3 per round)" % ROUNDS)
    old = H.HestonADI(0, lib_path=os.path.join(PARENT, "pde_based_heston_solver_gpu_accelerated_amd", "libhadi.so"))
    for m1, m2, n, N_do, N_jac in ((50, 25, 3000, 50, 20), (512, 256, 256, 20, 5)):
        strikes, g, gd, u0 = problem(m1, m2, n)
        u = torch.empty_like(u0)

        def plain(s):
            u.copy_(u0)
            s.DO_timestepping(m1, m2, N_do, T / N_do, THETA, R_D, R_F, *MODEL, gd, u)

        def jac(s):
            s.compute_jacobian_bates(*jac_args(m1, m2, N_jac, n, gd, u0))

        for name, fn, N in (("hadi_DO_timestepping", plain, N_do), ("hadi_compute_jacobian_bates", jac, N_jac)):
            (ma, mb), (sa, sb), (a, b) = alternate(lambda: fn(old), lambda: fn(sv))
            d_old, d_new = old.describe_last_sweep(), sv.describe_last_sweep()
            say("%s %dx%d x %d steps x %d: parent mean %.4f spread %.4f | new mean %.4f spread %.4f | new - parent %+.4f ms (%+.2f %%): %s" % (
                name, m1, m2, N, n, ma, sa, mb, sb, mb - ma, 100.0 * (mb - ma) / ma, verdict(ma, mb, sa)))
            say("    parent rounds %s" % " ".join("%.4f" % x for x in a))
            say("    new rounds    %s" % " ".join("%.4f" % x for x in b))
            say("    route: %s%s" % (d_new[:200], "" if d_new == d_old else "  [PARENT: %s]" % d_old[:200]))
    old.close()


def part_bc(sv):
    say("## (b) eight columns (9 groups, 3 matrix sets) beside five (6 groups, 1 set), per-instance matrices, device-resident inputs, "
        "lambda %g mu_J %g sigma_J %g; (c) strip sharing on / off" % JUMPS)
    N = 20
    for m1, m2, n in ((50, 25, 500), (256, 128, 64)):
        strikes, g, gd, u0 = problem(m1, m2, n)
        args = jac_args(m1, m2, N, n, gd, u0)
        five = lambda: sv.compute_jacobian_bates(*args)
        eight = lambda: sv.compute_jacobian_bates_jumps(*args)

        def eight_unshared():
            sv.set_tuning("jump_share", 0)
            try:
                sv.compute_jacobian_bates_jumps(*args)
            finally:
                sv.set_tuning("jump_share", 1)

        (m5, m8), (s5, s8), (r5, r8) = alternate(five, eight)
        d8 = sv.describe_last_sweep()
        say("%dx%d x %d steps x %d: five columns mean %.3f spread %.3f ms | eight columns mean %.3f spread %.3f ms | ratio %.3f "
            "(9 / 6 groups = 1.5)" % (m1, m2, N, n, m5, s5, m8, s8, m8 / m5))
        say("    five  rounds %s" % " ".join("%.3f" % x for x in r5))
        say("    eight rounds %s" % " ".join("%.3f" % x for x in r8))
        say("    %s" % d8[:320])
        sv.set_profiling(1)
        prof = {}
        for name, fn in (("five", five), ("eight", eight)):
            fn()
            rs = []
            for _ in range(3):
                fn()
                rs.append(sv.timing())
            prof[name] = (min(t["setup_ms"] for t in rs), min(t["sweep_ms"] for t in rs))
        sv.set_profiling(0)
        say("    under profiling: set-up (staging, v-grids, matrix build) five %.4f ms, eight %.4f ms (+%.4f ms for two more matrix sets: "
            "%.1f -> %.1f MB of entries); sweep five %.3f ms, eight %.3f ms (ratio %.3f)" % (
                prof["five"][0], prof["eight"][0], prof["eight"][0] - prof["five"][0], n * 8.0 * (m1 + 1) ** 2 / 1e6,
                3 * n * 8.0 * (m1 + 1) ** 2 / 1e6, prof["five"][1], prof["eight"][1], prof["eight"][1] / prof["five"][1]))
        (mu, ms), (su, ss), (ru, rs_) = alternate(eight_unshared, eight, rounds=ROUNDS + 2)
        say("    (c) eight columns, one instance per block mean %.3f spread %.3f ms | strips shared mean %.3f spread %.3f ms | shared - "
            "unshared %+.3f ms (%+.2f %%): %s" % (mu, su, ms, ss, ms - mu, 100.0 * (ms - mu) / mu, verdict(mu, ms, max(su, ss))))
        say("        unshared rounds %s" % " ".join("%.3f" % x for x in ru))
        say("        shared rounds   %s" % " ".join("%.3f" % x for x in rs_))


def part_d(sv):
    say("## (d) one LM iteration on 500 strikes of 50x25, 20 steps, device-resident inputs, wall ms (best of 3)")
    m1, m2, n, N = 50, 25, 500, 20
    strikes, g, gd, u0 = problem(m1, m2, n)
    ws = H.DOWorkspace(n, (m1 + 1) * (m2 + 1), device=DEV)
    ws.U.copy_(u0)
    market = sv.compute_base_prices_bates(S_0, V_0, R_D, R_F, *MODEL, m1, m2, (m1 + 1) * (m2 + 1), N, THETA, T / N, n, gd, ws,
                                          *JUMPS).cpu().numpy()
    start = (1.65, 0.036, 0.33, -0.81, 0.04)
    kw = dict(max_iter=1, tol=1e-12)
    head = lambda: (sv, S_0, T, R_D, R_F) + start + (m1, m2, N, THETA, gd, u0, market)
    runs = (("calibrate_european (5 parameters, no jumps)", lambda: H.calibrate_european(*head(), **kw)),
            ("calibrate_bates (5 parameters, the law held fixed)", lambda: H.calibrate_bates(*head(), *JUMPS, **kw)),
            ("calibrate_bates_jumps (8 parameters)", lambda: H.calibrate_bates_jumps(*head(), 0.65, -0.12, 0.12, **kw)))
    for name, fn in runs:
        res = fn()
        say("%s: %.3f ms per iteration (%d sweeps; sum r^2 %.3e -> %.3e)" % (
            name, timed(fn), res["pde_solves"] + n, res["history"][0]["error"], res["history"][0].get("trial_error", float("nan"))))


sv = H.HestonADI(0)
say("device %s" % sv.device_info())
if PARENT:
    part_a(sv)
else:
    say("## (a) existing calls: no --parent PARENT_TREE given, not measured")
part_bc(sv)
part_d(sv)
sv.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
