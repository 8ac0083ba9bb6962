#!/usr/bin/env python3
"""Diagnostic (needs a GPU): what the knock-out barrier entry points cost, and that the other calls cost what they did.
    python tools/barrier_ab.py [--parent PARENT_TREE] [--runs R] [--out FILE] [--skip-regs | --regs-only]
(a) Non-barrier calls, this tree against PARENT_TREE (a built checkout of the commit before; skipped without --parent): bench.py
    --full as a child process of each tree, R alternating runs each (default 5).  Per figure -- the headline (point-steps/s),
    other_workloads.c4 (ms per LM iteration), reference_harness (wall ms: European x1 and x500, American + dividends x500) -- both
    means and spreads (max - min); a difference of the means beyond the larger spread is flagged.  Then the registers and spills
    of every whole-loop kernel and of the barrier kernels (tools/kernel_regs.py: a compilation, no GPU needed -- --regs-only
    prints that section alone, --skip-regs leaves it out).
(b) The knock-out: a double barrier at 0.7 K and 1.3 K monitored on EVERY step against the European put on the same route, wall ms
    per call (best of 3 after a warm-up): 512x256 x 1000 steps x 256 instances on the streaming kernels (small_grid, team_launch
    and resident_sweep pinned to 0 for both calls, so that the route difference is not counted), there also under
    hadi_set_profiling -- hadi_knockout_kernel's time is the difference of the two sweeps over its launches, set against the 8 TB/s
    roofline at 8 B per knocked node and against the same run's column-pass time per step -- and 50x25 x 40 steps x 3000 instances
    on hadi_small_seq_kernel against the same kernel without monitoring.
The text goes to stdout and to FILE (default profiles/barrier_ab.txt)."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def opt(name, default, conv=str):
    if name in sys.argv:
        k = sys.argv.index(name)
        v = conv(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        return v
    return default


PARENT, RUNS = opt("--parent", None), opt("--runs", 5, int)
SKIP_REGS, REGS_ONLY = "--skip-regs" in sys.argv, "--regs-only" in sys.argv
OUT = opt("--out", os.path.join(ROOT, "profiles", "barrier_ab.txt"))
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def bench(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"],
                         cwd=tree, capture_output=True, text=True, timeout=900)
    if out.returncode:
        raise RuntimeError("bench.py failed in %s: %s" % (tree, out.stderr[-2000:]))
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    h = j["reference_harness"]
    return {"headline point-steps/s": j["value"], "c4 ms per LM iteration": j["other_workloads"]["c4"]["ms_per_iteration"],
            "harness EU x1 wall ms": h["european"]["1"]["wall_ms"], "harness EU x500 wall ms": h["european"]["500"]["wall_ms"],
            "harness AM+DIV x500 wall ms": h["american_dividend"]["500"]["wall_ms"]}


def part_a():
    say("## (a) non-barrier calls: bench.py --full, %d alternating runs, this tree against the parent commit's" % RUNS)
    new, old = [], []
    for r in range(RUNS):
        old.append(bench(PARENT))
        new.append(bench(ROOT))
        print("run %d: parent %s | new %s" % (r, list(old[-1].values()), list(new[-1].values())), flush=True)
    for key in new[0]:
        a, b = [x[key] for x in old], [x[key] for x in new]
        ma, mb = statistics.mean(a), statistics.mean(b)
        sa, sb = max(a) - min(a), max(b) - min(b)
        worse = (mb < ma) if "point-steps" in key else (mb > ma)
        verdict = "within the runs' spread" if abs(mb - ma) <= max(sa, sb) else ("SLOWER BEYOND THE SPREAD" if worse else "faster beyond the spread")
        say("%-30s parent mean %.6g spread %.3g | new mean %.6g spread %.3g | new - parent %+.3g (%+.2f %%): %s" % (
            key, ma, sa, mb, sb, mb - ma, 100.0 * (mb - ma) / ma, verdict))
        say("%-30s   parent runs %s" % ("", " ".join("%.6g" % x for x in a)))
        say("%-30s   new runs    %s" % ("", " ".join("%.6g" % x for x in b)))


def part_regs():
    from tools import kernel_regs
    say("## registers of the whole-loop kernels and of the barrier kernels (tools/kernel_regs.py; hipcc -O3, gfx950)")
    for dn, v, sg, sp, scr, lds in sorted(kernel_regs.collect()[0]):
        if any(f in dn for f in ("hadi_small", "hadi_knockout", "hadi_barrier_locate")):
            say("%-72s vgpr %3d sgpr %3d spill %d scratch %d B static LDS %d B" % (dn[:72], v, sg, sp, scr, lds))


def part_b():
    import numpy as np
    import torch
    import pde_based_heston_solver_gpu_accelerated_amd as H
    dev = torch.device("cuda:0")
    S_0, V_0, T, R_D, R_F, THETA = 100.0, 0.04, 1.0, 0.025, 0.0, 0.8
    MODEL = (-0.9, 0.3, 1.5, 0.04)
    sv = H.HestonADI(0)
    say("## (b) a double barrier (0.7 K, 1.3 K) monitored on every step against none (European), puts, device-resident inputs; device %s"
        % sv.device_info())

    def timed(fn, reps=3):
        fn()
        best = 1e30
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    shapes = ((512, 256, 1000, 256, {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}, {"small_grid": 1, "team_launch": -1, "resident_sweep": -1}),
              (50, 25, 40, 3000, {"small_seq": 1, "small_pairs": 0}, {"small_seq": -1, "small_pairs": -1}))
    for m1, m2, N, n, pin, unpin in shapes:
        strikes = [85.0 + 30.0 * k / (n - 1) for k in range(n)]
        g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
        k = np.asarray(strikes)
        lower, upper = 0.7 * k, 1.3 * k
        knocked = float(((g.Vec_s <= lower[:, None]) | (g.Vec_s >= upper[:, None])).mean())
        u0 = torch.from_numpy(g.put_payoff(strikes)).to(dev)
        gd, u = g.to(dev), torch.empty_like(u0)
        mon = list(range(1, N + 1))
        kw = dict(option_type=H.PUT, strikes=strikes)
        for key, val in pin.items():
            sv.set_tuning(key, val)

        def eu():
            u.copy_(u0)
            sv.DO_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u, **kw)

        def ko():
            u.copy_(u0)
            sv.barrier_timestepping(m1, m2, N, T / N, THETA, R_D, R_F, *MODEL, gd, u, mon, lower=lower, upper=upper, **kw)

        te = timed(eu)
        de = sv.describe_last_sweep()
        tb = timed(ko)
        db = sv.describe_last_sweep()
        say("%dx%d x %d steps x %d, %.1f %% of the nodes knocked: European %.3f ms, knock-out on every step %.3f ms: %+.3f ms (%+.2f %%)" % (
            m1, m2, N, n, 100.0 * knocked, te, tb, tb - te, 100.0 * (tb - te) / te))
        say("    European:  %s" % de[:150])
        say("    knock-out: %s" % db[:240])
        if m1 >= 512:
            sv.set_profiling(1)
            sw = {}
            for name, fn in (("eu", eu), ("ko", ko)):
                fn()
                runs = []
                for _ in range(3):
                    fn()
                    runs.append(sv.timing())
                sw[name] = min(runs, key=lambda t: t["sweep_ms"])
            sv.set_profiling(0)
            per_launch = (sw["ko"]["sweep_ms"] - sw["eu"]["sweep_ms"]) / len(mon)
            nbytes = 8.0 * knocked * n * (m1 + 1) * (m2 + 1)
            col = sw["ko"]["pass_b_ms"] / max(1, sw["ko"]["pass_b_launches"])
            say("    under profiling (the same streaming kernels launch by launch): sweep European %.3f ms, knock-out %.3f ms" % (
                sw["eu"]["sweep_ms"], sw["ko"]["sweep_ms"]))
            say("    hadi_knockout_kernel: %.4f ms per launch = %.0f GB/s at 8 B per knocked node = %.3f of the 8 TB/s roofline; the same "
                "run's column pass: %.4f ms per step (row pass %.4f)" % (
                    per_launch, nbytes / (per_launch * 1e-3) / 1e9 if per_launch > 0 else float("nan"),
                    nbytes / (per_launch * 1e-3) / 8e12 if per_launch > 0 else float("nan"), col,
                    sw["ko"]["pass_a_ms"] / max(1, sw["ko"]["pass_a_launches"])))
        for key, val in unpin.items():
            sv.set_tuning(key, val)
    sv.close()


if REGS_ONLY:
    part_regs()
else:
    if PARENT:
        part_a()
    else:
        say("## (a) non-barrier calls: no --parent PARENT_TREE given, not measured")
    if not SKIP_REGS:
        part_regs()
    part_b()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
