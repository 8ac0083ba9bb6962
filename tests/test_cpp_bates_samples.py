"""hadi_host::bates_sample_ladder, compute_base_prices_bates_samples and compute_jacobian_bates_samples (include/hadi_host.hpp) compile
and link against the C ABI with plain g++, and -- on a GPU -- return what the same calls through the Python mirror return, to the
last bit (two 50x25 instances of calls, three snapshots, three samples, per-instance jump laws; the Jacobian with eight and with
five columns)."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_host_bates_samples")


def _build():
    G.build_libhadi()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_host_bates_samples.cpp"), "-o", EXE,
                           "-L", PKG, "-lhadi", "-Wl,-rpath," + PKG])
    return EXE


def test_cpp_bates_samples_compiles_and_links_against_the_c_abi():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_bates_samples_reproduces_the_python_calls_bit_for_bit(solver):
    import pde_based_heston_solver_gpu_accelerated_amd as H
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0 and "all C++ Bates surface checks passed" in out.stdout

    def row(tag):
        (ln,) = [ln for ln in out.stdout.splitlines() if ln.startswith(tag + " ")]
        return np.array([float.fromhex(x) for x in ln.split()[2:]])
    S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, theta = 100.0, 0.04, 1.0, 0.025, 0.0, -0.9, 0.3, 1.5, 0.04, 0.8
    m1, m2, N = 50, 25, 8
    size = (m1 + 1) * (m2 + 1)
    strikes = [100.0, 105.0]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    U0 = grids.call_payoff(strikes)
    spots, scales, snaps = [S_0, 90.0, 110.5], [1.0, 1.1, 0.9], [2, 5, 8]
    law = ([0.5, 2.0], [-0.10, -0.05], [0.15, 0.10])
    lad = solver.bates_sample_ladder(m1, m2, N, T / N, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U0.copy(), spots, V_0, snaps, *law,
                                     scales=scales)
    ws = H.DOWorkspace(2, size)
    ws.U[...] = U0
    head = (spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, size, N, theta, T / N, 2, grids)
    base = solver.compute_base_prices_bates_samples(*head, ws, snaps, *law, scales=scales)
    J8, b8 = solver.compute_jacobian_bates_samples(*head, U0.copy(), snaps, *law, jump_columns=True, scales=scales, eps=1e-6)
    J5, b5 = solver.compute_jacobian_bates_samples(*head, U0.copy(), snaps, *law, scales=scales, eps=1e-6)
    assert lad.shape == (2, 3, 3) and J8.shape == (2, 3, 3, 8) and J5.shape == (2, 3, 3, 5)
    assert np.array_equal(row("LADDER"), lad.reshape(-1)) and np.array_equal(row("BASE"), base.reshape(-1))
    assert np.array_equal(row("JAC8"), J8.reshape(-1)) and np.array_equal(row("BASE8"), b8.reshape(-1))
    assert np.array_equal(row("JAC5"), J5.reshape(-1)) and np.array_equal(row("BASE5"), b5.reshape(-1))
