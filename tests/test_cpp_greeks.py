"""hadi_host::compute_greeks (include/hadi_host.hpp) compiles and links against the C ABI with plain g++, and -- on a GPU --
returns the [n][8] of the same call through the Python mirror, to the last bit (one 50x25 batch of American puts with
dividends)."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_host_greeks")


def _build():
    G.build_libhadi()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_host_greeks.cpp"), "-o", EXE,
                           "-L", PKG, "-lhadi", "-Wl,-rpath," + PKG])
    return EXE


def test_cpp_greeks_compiles_and_links_against_the_c_abi():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_greeks_reproduce_the_python_call_bit_for_bit(solver):
    import pde_based_heston_solver_gpu_accelerated_amd as H
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0 and "all C++ Greeks checks passed" in out.stdout
    rows = [ln.split()[2:] for ln in out.stdout.splitlines() if ln.startswith("GREEKS ")]
    cpp = np.array([[float.fromhex(x) for x in r] for r in rows])
    S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, theta = 100.0, 0.04, 1.0, 0.025, 0.007, -0.9, 0.3, 1.5, 0.04, 0.8
    m1, m2, N = 50, 25, 20
    strikes = [90.0, 95.0, 100.0, 105.0]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    U = grids.put_payoff(strikes)
    div = H.Dividends([0.2, 0.4, 0.6, 0.8], [0.5, 0.3, 0.2, 0.1], [0.02] * 4)
    py = solver.compute_greeks(m1, m2, N, T / N, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, S_0, V_0,
                               variant=H.AM_DIV, dividends=div, option_type=H.PUT, strikes=strikes)
    assert cpp.shape == (4, 8) and py.shape == (4, 8)
    assert np.array_equal(cpp, py), (cpp, py)
    assert (py[:, H.G_PRICE] > 0).all() and (py[:, H.G_DELTA] < 0).all() and (py[:, H.G_GAMMA] > 0).all()
