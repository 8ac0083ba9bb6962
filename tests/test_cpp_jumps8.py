"""hadi_host::compute_jacobian_bates_jumps, lm_partials_n and lm_solve_n (include/hadi_host.hpp) compile and link against the C ABI
with plain g++, and -- on a GPU -- return what the same calls through the Python mirror return, to the last bit (one 50x25 batch
of puts with dividends: per-instance jump laws, then one shared law, then the 73 partial sums and one LM step)."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "test_host_jumps8")


def _build():
    G.build_libhadi()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_host_jumps8.cpp"), "-o", EXE,
                           "-L", PKG, "-lhadi", "-Wl,-rpath," + PKG])
    return EXE


def test_cpp_jumps8_compiles_and_links_against_the_c_abi():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_jumps8_reproduces_the_python_calls_bit_for_bit(solver):
    import pde_based_heston_solver_gpu_accelerated_amd as H
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0 and "all C++ eight-column checks passed" in out.stdout

    def rows(tag):
        return np.array([[float.fromhex(x) for x in ln.split()[2:]] for ln in out.stdout.splitlines() if ln.startswith(tag + " ")])
    S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, theta = 100.0, 0.04, 1.0, 0.025, 0.007, -0.9, 0.3, 1.5, 0.04, 0.8
    m1, m2, N = 50, 25, 20
    size = (m1 + 1) * (m2 + 1)
    strikes = [90.0, 95.0, 100.0, 105.0]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    U0 = grids.put_payoff(strikes)
    div = H.Dividends([0.2, 0.4, 0.6, 0.8], [0.5, 0.3, 0.2, 0.1], [0.02] * 4)
    per = {"option_type": H.PUT, "strikes": strikes}
    head = (S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, size, N, theta, T / N, 4, grids)
    kw = dict(eps=1e-6, variant=H.DIV, dividends=div, per_instance=per)
    Jp, bp = solver.compute_jacobian_bates_jumps(*head, U0.copy(), [0.5, 2.0, 0.0, 0.3], [-0.10, -0.05, 0.0, 0.10], [0.15, 0.10, 0.2, 0.30],
                                                 **kw)
    J, b = solver.compute_jacobian_bates_jumps(*head, U0.copy(), 0.5, -0.10, 0.15, **kw)
    assert Jp.shape == (4, 8) and np.array_equal(rows("JACP"), Jp) and np.array_equal(rows("BASEP")[:, 0], bp)
    assert np.array_equal(rows("JAC"), J) and np.array_equal(rows("BASE")[:, 0], b)
    resid = np.array([0.05 * (i + 1) - 0.1 for i in range(4)])
    part = H.lm_partials(J, resid)
    assert part.shape == (73,) and np.array_equal(rows("PART")[0], part)
    assert np.array_equal(rows("DELTA")[0], H.lm_solve(part, 0.01))
