#!/usr/bin/env python3
"""Diagnostic (GPU, not product): where a wavefront of hadi_sweep_resident<8> spends a time step.  Builds libhadi with
-DHADI_STAMPS=5 into tools/_stamps/ and runs one 20-step, 256-instance 512x256 sweep on it.  Prints shader-clock cycles per
piece and step, averaged over the blocks' wavefronts.
    python tools/resident_stamps.py [out.txt]     (--build-only: compile, run nothing; --no-build: use what is there)
The stamps serialise the scalar pipe at seven points per step: the shares are what to read, not the absolute speed."""
import ctypes as C, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
out = os.path.join(ROOT, "tools", "_stamps"); os.makedirs(out, exist_ok=True)
VARIANTS = [("product schedule", "libhadi_res.so", [])]
NAMES = ["row prologue (to its second barrier)", "row loop", "retire + block meets", "column prologue (to the first solve)",
         "full column tiles", "short column tile", "final retire + block meets"]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--no-build" not in sys.argv:
    for _, so, flags in VARIANTS:
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared", "-DHADI_STAMPS=5", *flags, "-o",
                               os.path.join(out, so), os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc", "hadi_api.hip")])
if "--build-only" in sys.argv:
    sys.exit(0)
if len(args) > 1:  # child: one variant per process (one libhadi per process)
    import pde_based_heston_solver_gpu_accelerated_amd._native as nat
    nat.LIB_PATH = args[1]
    import pde_based_heston_solver_gpu_accelerated_amd as H
    import torch
    n, N, m1, m2 = 256, 20, 512, 256
    strikes = [85 + 30 * k / (n - 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, 100.0, 0.04, strikes); U0 = g.call_payoff(strikes)
    dev = torch.device("cuda:0"); gd = g.to(dev); U = torch.from_numpy(U0).to(dev)
    s = H.HestonADI(0)
    L = nat.lib(); L.hadi_debug_stamps.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 32)()
    L.hadi_debug_stamps(buf, 1)
    s.DO_timestepping(m1, m2, N, 1.0 / 1000, 0.8, 0.025, 0.0, -0.9, 0.3, 1.5, 0.04, gd, U)
    assert "hadi_sweep_resident<8>" in s.describe_last_sweep(), s.describe_last_sweep()
    L.hadi_debug_stamps(buf, 1)
    waves = n * 8 * N
    tot = sum(buf[k] for k in range(7))
    print("sweep_ms %.3f (stamped build), %d cycles per step" % (s.timing()["sweep_ms"], tot // waves))
    for k, nm in enumerate(NAMES):
        print("  %-40s %9.0f cycles/step  %5.1f %%" % (nm, buf[k] / waves, 100.0 * buf[k] / tot))
    sys.exit(0)
lines = ["# Phase stamps of hadi_sweep_resident<8> (tools/resident_stamps.py): 256 instances of 512x256, 20 steps, one sweep;",
         "# shader-clock (s_memtime) cycles per piece and step, averaged over the 2048 wavefronts of the launch."]
for title, so, _ in VARIANTS:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-build", "child", os.path.join(out, so)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit("%s failed (%d):\n%s" % (title, r.returncode, r.stderr[-2000:]))
    lines += ["%s:" % title] + r.stdout.rstrip().splitlines()
text = "\n".join(lines) + "\n"
print(text, end="")
if args:
    open(args[0], "w").write(text)
