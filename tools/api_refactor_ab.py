#!/usr/bin/env python3
"""Diagnostic (needs a GPU): this tree against a built checkout of the commit before, on the host-bound figures -- what a change
of the drivers of csrc/hadi_api.hip and of the launchers of solver.py can move.
    python tools/api_refactor_ab.py --parent PARENT_TREE [--runs R] [--raw FILE] [--out FILE]
R rounds (default 5), parent first in the odd ones and second in the even ones, as tools/small_refactor_ab.py has them.  A round
is, per side, two child processes that import the side's own package and load the side's own libhadi.so: bench.py --full in the
side's tree -- the headline (point-steps/s), other_workloads.c4 (ms per LM iteration) and every row of reference_harness (wall ms)
-- and this file with --latency TREE: the median wall ms per call over 40 calls (after 3) of each case of tools/api_trace_cases.py,
one per driver and feature (Jacobian, Jacobian ladder, sampled Jacobian, Bermudan base prices with a schedule per instance on the
streaming route, barrier base prices, Greeks with the spot ladder).  Every round is appended to the raw file (JSON lines), so the
rounds may be spread over several calls; the report is made from all rounds in it.  A figure passes where the new side's median
lies inside the parent's own min .. max, or on the better side of it.
The text goes to stdout and to FILE (default build/api_refactor_ab.txt, the raw rounds beside it: build/ is not tracked.
profiles/api_refactor_ab.txt is a recorded run with notes written by hand, which this tool never writes)."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opt(name, default, conv=str):
    if name in sys.argv:
        k = sys.argv.index(name)
        v = conv(sys.argv[k + 1])
        del sys.argv[k:k + 2]
        return v
    return default


def latency(tree):
    """(child process) The cases of tools/api_trace_cases.py on the package and the library of `tree`: one JSON line."""
    sys.path.insert(0, tree)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import pde_based_heston_solver_gpu_accelerated_amd as H
    import api_trace_cases as A
    row = {}
    for case in A.CASES:
        with H.HestonADI(0) as sv:
            call = A.prepare(H, sv, case)
            for _ in range(3):
                call()
            ts = []
            for _ in range(40):
                t0 = time.perf_counter()
                call()
                ts.append(1e3 * (time.perf_counter() - t0))
            row["%s ms per call" % case] = statistics.median(ts)
    print(json.dumps(row))


def child(tree, argv, timeout):
    out = subprocess.run([sys.executable] + argv, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if out.returncode:
        raise RuntimeError("%s failed in %s: %s" % (argv, tree, out.stderr[-2000:]))
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def bench(tree):
    j = child(tree, ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"], 900)
    h = j["reference_harness"]
    row = {"headline point-steps/s": j["value"], "c4 ms per LM iteration": j["other_workloads"]["c4"]["ms_per_iteration"]}
    for n, v in h["european"].items():
        row["harness EU x%s wall ms" % n] = v["wall_ms"]
    for n, v in h["american_dividend"].items():
        row["harness AM+DIV x%s wall ms" % n] = v["wall_ms"]
    for n in ("1", "500"):  # (the sweep's own time between its two events: what of a wall figure is not the host's)
        row["harness EU x%s kernel ms" % n] = h["european"][n]["kernel_ms"]
    return row


def main():
    parent, runs = opt("--parent", None), opt("--runs", 5, int)
    if parent is None:
        sys.exit(__doc__)
    parent = os.path.abspath(parent)
    out_path = opt("--out", os.path.join(ROOT, "build", "api_refactor_ab.txt"))
    raw = opt("--raw", out_path + ".raw.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for r in range(runs):
        for side, tree in (("parent", parent), ("new", ROOT))[::1 if r % 2 == 0 else -1]:
            row = {"side": side, **bench(tree), **child(tree, [os.path.abspath(__file__), "--latency", tree], 300)}
            with open(raw, "a") as f:
                f.write(json.dumps(row) + "\n")
            print("round %d %s done" % (r + 1, side), flush=True)
    rows = [json.loads(ln) for ln in open(raw)]
    old, new = [x for x in rows if x["side"] == "parent"], [x for x in rows if x["side"] == "new"]
    lines = ["## this tree against the parent commit's: bench.py --full and the call latencies of tools/api_trace_cases.py, %d alternating rounds" % len(new),
             "## a figure passes where the new median lies inside the parent's own min .. max, or beyond it on the better side"]
    for key in [k for k in new[0] if k != "side"]:
        a, b = [x[key] for x in old], [x[key] for x in new]
        mb, lo, hi = statistics.median(b), min(a), max(a)
        higher_is_better = "point-steps" in key
        verdict = "inside" if lo <= mb <= hi else ("better than every parent run" if (mb > hi) == higher_is_better else "SLOWER THAN EVERY PARENT RUN")
        lines.append("%-34s parent min %.6g median %.6g max %.6g | new median %.6g (%+.2f %% of the parent's): %s"
                     % (key, lo, statistics.median(a), hi, mb, 100.0 * (mb / statistics.median(a) - 1.0), verdict))
        lines.append("%-34s   parent runs %s" % ("", " ".join("%.6g" % x for x in a)))
        lines.append("%-34s   new runs    %s" % ("", " ".join("%.6g" % x for x in b)))
    print("\n".join(lines))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--latency" in sys.argv:
        latency(sys.argv[sys.argv.index("--latency") + 1])
    else:
        main()
