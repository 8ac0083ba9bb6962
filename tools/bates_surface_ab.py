#!/usr/bin/env python3
"""Diagnostic (needs a GPU): what a Bates strike x maturity surface costs, per call, and which route the new call should take.
    python tools/bates_surface_ab.py [--rounds R] [--out FILE]
A surface is 10 maturities (10, 20, .. 100 steps of one delta_t) at 50 and at 500 strikes; the calls are the eight-column Jacobian
and the base prices, device-resident inputs, wall ms per call around a device synchronise (best of 3 in every round, R alternating
rounds, default 5; the spread is max - min of the rounds' values).
(a) What the library could do before the surface calls: one compute_jacobian_bates_jumps / compute_base_prices_bates call per maturity,
    one 50x25 instance per strike; the ten calls are timed together.
(b) compute_jacobian_bates_samples / compute_base_prices_bates_samples on the streaming route ("jump_small" = 0): ONE instance on
    50x25, on 100x20 and on 100x50.
(c) The same calls on hadi_small_jump_kernel ("jump_small" = 1) on 50x25 and on 100x20 (two nodes per lane), alternating with (b).
(d) The batch size: hadi_bates_sample_ladder with 1 .. 4096 instances of 50x25 and 1 .. 2048 of 100x20 on both routes, alternating --
    what the automatic rule of "jump_small" is read off.
The text goes to stdout and to FILE (default profiles/bates_surface_ab.txt)."""
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


ROUNDS = opt("--rounds", 5, int)
OUT = opt("--out", os.path.join(ROOT, "profiles", "bates_surface_ab.txt"))
LINES = []

import numpy as np
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

DEV = torch.device("cuda:0")
S_0, V_0, R_D, R_F, THETA = 100.0, 0.04, 0.025, 0.0, 0.8
MODEL = (-0.9, 0.3, 1.5, 0.04)
JUMPS = (0.5, -0.10, 0.15)
BASE_STRIKE = 100.0
SNAPS = list(range(10, 101, 10))
DT = 1.0 / 100


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


def alternate(fns):
    """R alternating rounds of several calls: per call (mean, spread, rounds)."""
    for f in fns:
        f()
    rs = [[] for _ in fns]
    for _ in range(ROUNDS):
        for k, f in enumerate(fns):
            rs[k].append(timed(f))
    return [(statistics.mean(r), max(r) - min(r), r) for r in rs]


def strikes_of(n):
    return [80.0 + 45.0 * k / (n - 1) for k in range(n)]


def routed(sv, route, fn):
    def run():
        sv.set_tuning("jump_small", route)
        try:
            return fn()
        finally:
            sv.set_tuning("jump_small", -1)
    return run


def part_a(sv):
    say("## (a) one call per maturity, one 50x25 instance per strike (compute_jacobian_bates_jumps / compute_base_prices_bates), ten calls together")
    m1, m2 = 50, 25
    size = (m1 + 1) * (m2 + 1)
    out = {}
    for n in (50, 500):
        strikes = strikes_of(n)
        g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
        gd, u0 = g.to(DEV), torch.from_numpy(g.call_payoff(strikes)).to(DEV)
        ws = H.DOWorkspace(n, size, device=DEV)

        def jac():
            for N in SNAPS:
                sv.compute_jacobian_bates_jumps(S_0, V_0, R_D, R_F, *MODEL, m1, m2, size, N, THETA, DT, n, gd, u0, *JUMPS)

        def base():
            for N in SNAPS:
                ws.U.copy_(u0)
                sv.compute_base_prices_bates(S_0, V_0, R_D, R_F, *MODEL, m1, m2, size, N, THETA, DT, n, gd, ws, *JUMPS)

        (mj, sj, rj), (mb, sb, rb) = alternate([jac, base])
        out[n] = (mj, mb)
        say("%d strikes: Jacobian (8 columns) mean %.3f spread %.3f ms | base prices mean %.3f spread %.3f ms   [%s]" % (
            n, mj, sj, mb, sb, sv.describe_last_sweep()[:110]))
        say("    Jacobian rounds %s | base rounds %s" % (" ".join("%.3f" % x for x in rj), " ".join("%.3f" % x for x in rb)))
    return out


def surface_calls(sv, m1, m2, n_strikes):
    size = (m1 + 1) * (m2 + 1)
    g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, [BASE_STRIKE])
    gd, u0 = g.to(DEV), torch.from_numpy(g.call_payoff([BASE_STRIKE])).to(DEV)
    spots, scales = H.strike_samples(S_0, BASE_STRIKE, strikes_of(n_strikes))
    ws = H.DOWorkspace(1, size, device=DEV)
    ws.U.copy_(u0)
    head = (spots, V_0, R_D, R_F) + MODEL + (m1, m2, size, SNAPS[-1], THETA, DT, 1, gd)
    jac = lambda: sv.compute_jacobian_bates_samples(*head, u0, SNAPS, *JUMPS, jump_columns=True, scales=scales)
    base = lambda: sv.compute_base_prices_bates_samples(*head, ws, SNAPS, *JUMPS, scales=scales)
    return jac, base


def part_bc(sv, before):
    say("## (b) the surface calls on the streaming route, (c) on hadi_small_jump_kernel; ONE instance, 10 snapshots x the strikes as samples")
    verdicts = {}
    for m1, m2 in ((50, 25), (100, 20), (100, 50)):
        for n in (50, 500):
            jac, base = surface_calls(sv, m1, m2, n)
            for name, fn, inst in (("Jacobian (8 columns)", jac, 9), ("base prices", base, 1)):
                fs = routed(sv, 0, fn)
                fs()
                ds = sv.describe_last_sweep()
                if m1 == 100 and m2 == 50:  # (the block kernel does not admit it)
                    ((ms, ss, rs),) = alternate([fs])
                    say("%dx%d, %d strikes, %s: streaming mean %.3f spread %.3f ms  (a) %.3f ms" % (m1, m2, n, name, ms, ss, before[n][inst == 1]))
                    continue
                fl = routed(sv, 1, fn)
                fl()
                dl = sv.describe_last_sweep()
                assert dl.startswith("hadi_small_jump_kernel<") and "row pass" in ds, (ds, dl)
                (ms, ss, rs), (ml, sl, rl) = alternate([fs, fl])
                spread = max(ss, sl)
                v = "whole-loop faster beyond the spread" if ms - ml > spread else ("streaming faster beyond the spread" if ml - ms > spread else "within the spread")
                verdicts[(m1, m2, inst, n)] = (ms, ml, spread, v)
                say("%dx%d, %d strikes, %s (%d instances): (b) streaming mean %.3f spread %.3f ms | (c) whole-loop mean %.3f spread %.3f ms | "
                    "(c) - (b) %+.3f ms: %s | (a) %.3f ms" % (m1, m2, n, name, inst, ms, ss, ml, sl, ml - ms, v, before[n][inst == 1]))
                say("    (b) rounds %s | (c) rounds %s" % (" ".join("%.3f" % x for x in rs), " ".join("%.3f" % x for x in rl)))
                say("    (b) %s" % ds[:260])
                say("    (c) %s" % dl[:260])
    return verdicts


def part_d(sv):
    say("## (d) hadi_bates_sample_ladder by batch size, 100 steps, 10 snapshots x 10 samples, per-instance matrices: streaming against whole-loop")
    N = 100
    cus = sv.device_info()["compute_units"]
    rows = []
    for m1, m2, sizes in ((50, 25, (1, 9, 16, 32, 64, 256, 512, 1024, 2048, 4096)), (100, 20, (1, 9, 64, 256, 512, 1024, 2048))):
        for n in sizes:
            strikes = [85.0 + 30.0 * k / max(n - 1, 1) for k in range(n)]
            g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
            gd, u0 = g.to(DEV), torch.from_numpy(g.call_payoff(strikes)).to(DEV)
            spots = np.linspace(85.0, 118.0, 10)
            fn = lambda: sv.bates_sample_ladder(m1, m2, N, DT, THETA, R_D, R_F, *MODEL, gd, u0, spots, V_0, SNAPS, *JUMPS)
            (ms, ss, rs), (ml, sl, rl) = alternate([routed(sv, 0, fn), routed(sv, 1, fn)])
            spread = max(ss, sl)
            v = "whole-loop faster beyond the spread" if ms - ml > spread else ("streaming faster beyond the spread" if ml - ms > spread else "within the spread")
            rows.append((m1, m2, n, ms, ml, spread, v))
            say("%dx%d %5d instances (%.3f per CU): streaming mean %.3f spread %.3f ms | whole-loop mean %.3f spread %.3f ms | %+.3f ms: %s" % (
                m1, m2, n, n / float(cus), ms, ss, ml, sl, ml - ms, v))
    return rows, cus


sv = H.HestonADI(0)
say("device %s" % (sv.device_info(),))
before = part_a(sv)
verdicts = part_bc(sv, before)
rows, cus = part_d(sv)
say("## the rule read off (b), (c) and (d)")
say("the surface driver's own batches (1 and 9 instances of ONE grid): %s" % "; ".join(
    "%dx%d x %d (%d strikes): %s" % (k[0], k[1], k[2], k[3], v[3]) for k, v in sorted(verdicts.items())))
for m1, m2 in sorted({(r[0], r[1]) for r in rows}):
    mine = [r for r in rows if (r[0], r[1]) == (m1, m2)]
    wins = [r[2] for r in mine if r[6].startswith("whole-loop")]
    rest = [r[2] for r in mine if not r[6].startswith("whole-loop")]
    say("%dx%d: whole-loop faster beyond the spread at %s instances, not so at %s" % (m1, m2, wins or "no", rest or "no"))
above = [r for r in rows if r[2] >= cus]
below = [r for r in rows if r[2] < cus]
say("the automatic rule of \"jump_small\" (hadi_route.h) is: hadi_small_jump_kernel for batches of at least one instance per CU (%d), streaming "
    "below.  At or above it the whole-loop kernel is faster beyond the spread at %d of the %d measured (grid, size) classes; below it at %d of %d, "
    "and at none of the surface driver's own batches of 1 and 9 instances -- so calibrate_bates_surface streams by default." % (
        cus, sum(r[6].startswith("whole-loop") for r in above), len(above), sum(r[6].startswith("whole-loop") for r in below), len(below)))
sv.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
