#!/usr/bin/env python3
"""Diagnostic (needs a GPU): what the forward-start / cliquet entry points cost, and that the plain calls cost what they did.
    python tools/cliquet_ab.py [--parent PARENT_TREE] [--rounds R] [--out FILE]
(1) Plain calls, this tree against PARENT_TREE (a built checkout of the commit before; skipped without --parent): hadi_DO_timestepping
    on 50x25 x 3000 (the whole-loop kernels, which carry one more hook) and on 512x256 x 256, both libraries loaded into this
    process, R alternating rounds (default 7), wall ms per call (best of 3 in every round).  The allowance is the spread
    (max - min) of the parent's own rounds; a difference of the means beyond it is flagged.
(2) A fixing step beside a plain step, on the streaming kernels (small_grid, team_launch and resident_sweep pinned to 0 for both
    calls) at 50x25, 256x128 and 512x256: a fixing on EVERY step, without and with weights, against the plain call; under
    hadi_set_profiling the two fixing kernels' time is the difference of the sweeps over the fixing steps, set against the same run's
    two passes per step and against the bytes moved at 8 B (+8 B with weights) per node.
(3) What the feature replaces: a four-period and a twelve-period cliquet (RETURN, weights 1) and a forward-start call (SHARES, one
    fixing at N / 2) at 50x25 x 500 and 256x128 x 64, 48 steps: one sweep against the host alternative on this commit -- the same
    steps as separate DO_timestepping calls, the field downloaded, rewritten in numpy and uploaded at every fixing.  Calls with
    r_f = 0 (time-independent boundary data), so both compute the same field: the largest difference is printed.
The text goes to stdout and to FILE (default profiles/cliquet_ab.txt)."""
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
OUT = opt("--out", os.path.join(ROOT, "profiles", "cliquet_ab.txt"))
LINES = []

import numpy as np
import torch
import pde_based_heston_solver_gpu_accelerated_amd as H

DEV = torch.device("cuda:0")
S_0, V_0, T, R_D, R_F, THETA = 100.0, 0.04, 1.0, 0.025, 0.0, 0.8
MODEL = (-0.9, 0.3, 1.5, 0.04)
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


def problem(m1, m2, n):
    strikes = [85.0 + 30.0 * k / (n - 1) for k in range(n)]
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
    say("## (2) a fixing on every step against none, streaming kernels, calls, device-resident inputs")
    for key, val in STREAMING.items():
        sv.set_tuning(key, val)
    for m1, m2, N, n in ((50, 25, 40, 3000), (256, 128, 40, 256), (512, 256, 40, 256)):
        strikes, g, gd, u0 = problem(m1, m2, n)
        u = torch.empty_like(u0)
        ref = np.array([g.Vec_s[k][int(np.argmin(np.abs(g.Vec_s[k] - strikes[k])))] for k in range(n)])
        steps = list(range(1, N + 1))
        nodes = float(n) * (m1 + 1) * (m2 + 1)

        def plain():
            u.copy_(u0)
            sv.DO_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u)

        def fixed(w):
            u.copy_(u0)
            sv.cliquet_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u, steps, ref, H.FIX_SHARES, w)

        runs = (("plain", plain, 0.0), ("no weights", lambda: fixed(None), 8.0), ("weights", lambda: fixed([1e-3] * N), 16.0))
        wall, prof = {}, {}
        for name, fn, _ in runs:
            fn()
            wall[name] = timed(fn)
        d = sv.describe_last_sweep()
        sv.set_profiling(1)
        for name, fn, _ in runs:
            fn()
            rs = []
            for _ in range(3):
                fn()
                rs.append(sv.timing())
            prof[name] = min(rs, key=lambda t: t["sweep_ms"])
        sv.set_profiling(0)
        say("%dx%d x %d steps x %d: plain %.3f ms, a fixing on every step %.3f ms (%+.2f %%), with weights %.3f ms (%+.2f %%)" % (
            m1, m2, N, n, wall["plain"], wall["no weights"], 100.0 * (wall["no weights"] / wall["plain"] - 1.0), wall["weights"],
            100.0 * (wall["weights"] / wall["plain"] - 1.0)))
        say("    %s" % d[:260])
        p = prof["plain"]
        row, col = p["pass_a_ms"] / max(1, p["pass_a_launches"]), p["pass_b_ms"] / max(1, p["pass_b_launches"])
        for name, _, bpn in runs[1:]:
            per = (prof[name]["sweep_ms"] - p["sweep_ms"]) / N
            say("    under profiling, %s: gather + apply %.4f ms per fixing step beside row pass %.4f + column pass %.4f ms per step (%.1f %% of "
                "a step); %.0f GB/s at %.0f B per node = %.3f of the 8 TB/s roofline" % (
                    name, per, row, col, 100.0 * per / (row + col), bpn * nodes / (per * 1e-3) / 1e9 if per > 0 else float("nan"), bpn,
                    bpn * nodes / (per * 1e-3) / 8e12 if per > 0 else float("nan")))
    for key, val in DEFAULT.items():
        sv.set_tuning(key, val)


def part_3(sv):
    say("## (3) one sweep against the host alternative (separate DO_timestepping calls; download, numpy rewrite, upload at every fixing), 48 steps")
    N = 48
    for m1, m2, n in ((50, 25, 500), (256, 128, 64)):
        strikes, g, gd, _ = problem(m1, m2, n)
        vs = g.Vec_s
        i_ref = [int(np.argmin(np.abs(vs[k] - S_0))) for k in range(n)]
        ref = np.array([vs[k][i_ref[k]] for k in range(n)])
        a_sh = vs / ref[:, None]
        coupon = H.local_return_payoff(g, ref, 1.0, 0.0, 0.05)
        fwd = np.ascontiguousarray(np.tile(np.maximum(vs - ref[:, None], 0.0), (1, m2 + 1)))
        contracts = (("four-period cliquet", coupon, [12, 24, 36], H.FIX_RETURN, 1.0), ("twelve-period cliquet", coupon, list(range(4, 48, 4)), H.FIX_RETURN, 1.0),
                     ("forward-start call", fwd, [24], H.FIX_SHARES, None))
        for name, pay, steps, mode, w in contracts:
            p0 = torch.from_numpy(pay).to(DEV)
            u = torch.empty_like(p0)
            res = {}

            def sweep():
                u.copy_(p0)
                sv.cliquet_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u, steps, ref, mode, None if w is None else [w] * len(steps))
                res["sweep"] = u

            def host():
                u.copy_(p0)
                prev = 0
                for s in steps + [N]:
                    sv.DO_timestepping(m1, m2, s - prev, T / N, THETA, R_D, R_F, *MODEL, gd, u)
                    prev = s
                    if s == N and N not in steps:
                        break
                    F = u.cpu().numpy().reshape(n, m2 + 1, m1 + 1)
                    c = F[np.arange(n), :, i_ref][:, :, None]
                    F = np.repeat(c, m1 + 1, axis=2) if mode == H.FIX_RETURN else c * a_sh[:, None, :]
                    if w is not None:
                        F = F + w * pay.reshape(n, m2 + 1, m1 + 1)
                    u.copy_(torch.from_numpy(np.ascontiguousarray(F.reshape(n, -1))).to(DEV))
                res["host"] = u

            sweep()
            d = sv.describe_last_sweep()
            a = u.cpu().numpy().copy()
            host()
            diff = np.abs(a - u.cpu().numpy()).max() / np.abs(a).max()
            ts, th = timed(sweep), timed(host)
            say("%dx%d x %d, %s (%d fixings): one sweep %.3f ms, host alternative %.3f ms: %.1fx; largest difference %.1e of max|U|" % (
                m1, m2, n, name, len(steps), ts, th, th / ts, diff))
            say("    %s" % d[:200])


sv = H.HestonADI(0)
say("device %s" % sv.device_info())
if PARENT:
    part_1(sv)
else:
    say("## (1) plain calls: no --parent PARENT_TREE given, not measured")
part_2(sv)
part_3(sv)
sv.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
