#!/usr/bin/env python3
"""Diagnostic (needs a GPU): this tree against a built checkout of the commit before, on the figures the small-grid LDS kernels
and the dividend kernels carry.
    python tools/small_refactor_ab.py --parent PARENT_TREE [--runs R] [--raw FILE] [--out FILE] [--sch-only]
R rounds (default 5), parent first in the odd ones and second in the even ones (two byte-identical libraries measured parent
first throughout differed by up to 0.5 % in their medians, second slower: profiles/small_refactor_ab.txt).  A round is, per side, bench.py --full as a child process of the tree -- the
headline (point-steps/s), other_workloads.c4 (ms per LM iteration: 3000 + 500 LDS-resident solves) and every row of
reference_harness (50x25x20 at 1 .. 500 instances European, 500 American + dividends; wall ms) -- and tools/schemes_bench.py
--lib on the side's libhadi.so: CS / MCS / HV on 50x25 x 3000, N = 100 (hadi_small_sch_kernel; sweep ms per step).  --sch-only
leaves bench.py out (a change that touches hadi_small_sch_kernel alone).  Every round is appended to the raw
file (JSON lines), so the rounds may be spread over several calls; the report is made from all rounds in it.  A figure passes
where the new side's median lies inside the parent's own min .. max (or on the better side of it).
The text goes to stdout and to FILE (default profiles/small_refactor_ab.txt)."""
import json, os, re, statistics, subprocess, sys
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
if PARENT is None:
    sys.exit(__doc__)
PARENT = os.path.abspath(PARENT)
SCH_ONLY = "--sch-only" in sys.argv
OUT = opt("--out", os.path.join(ROOT, "profiles", "small_refactor_ab.txt"))
RAW = opt("--raw", OUT + ".raw.jsonl")
PKG = "pde_based_heston_solver_gpu_accelerated_amd"


def bench(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"],
                         cwd=tree, capture_output=True, text=True, timeout=900)
    if out.returncode:
        raise RuntimeError("bench.py failed in %s: %s" % (tree, out.stderr[-2000:]))
    j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    h = j["reference_harness"]
    row = {"headline point-steps/s": j["value"], "c4 ms per LM iteration": j["other_workloads"]["c4"]["ms_per_iteration"]}
    for n, v in h["european"].items():
        row["harness EU x%s wall ms" % n] = v["wall_ms"]
    for n, v in h["american_dividend"].items():
        row["harness AM+DIV x%s wall ms" % n] = v["wall_ms"]
    return row


def schemes(lib):
    """CS / MCS / HV on 50x25 x3000, N = 100, from tools/schemes_bench.py (best of three, sweep ms per step) on the build `lib`."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "schemes_bench.py"), "--lib", lib, "3000", "100", "50", "25"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    if out.returncode:
        raise RuntimeError("schemes_bench.py failed on %s: %s" % (lib, out.stderr[-2000:]))
    row = {}
    for name, long_name in (("CS", "Craig-Sneyd"), ("MCS", "MCS"), ("HV", "HV")):
        m = re.search(r"^50x25 x3000 %s +([0-9.]+) ms per step.*\| (.*)$" % long_name, out.stdout, flags=re.M)
        assert m and "hadi_small_sch_kernel<1,%s>" % name in m.group(2), out.stdout
        row["sch %s 50x25 x3000 ms per step" % name] = float(m.group(1))
    return row


def main():
    for r in range(RUNS):
        for side, tree in (("parent", PARENT), ("new", ROOT))[::1 if r % 2 == 0 else -1]:
            row = {"side": side, **({} if SCH_ONLY else bench(tree)), **schemes(os.path.join(tree, PKG, "libhadi.so"))}
            with open(RAW, "a") as f:
                f.write(json.dumps(row) + "\n")
            print("round %d %s done" % (r + 1, side), flush=True)
    rows = [json.loads(ln) for ln in open(RAW)]
    old, new = [x for x in rows if x["side"] == "parent"], [x for x in rows if x["side"] == "new"]
    import pde_based_heston_solver_gpu_accelerated_amd as H
    with H.HestonADI(0) as sv:
        device = sv.device_info()
    lines = ["## this tree against the parent commit's: %sCS / MCS / HV on 50x25 x3000 (tools/schemes_bench.py), %d alternating rounds, device %s"
             % ("" if SCH_ONLY else "bench.py --full and ", len(new), device),
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
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
