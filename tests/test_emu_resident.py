"""CPU-only check of the resident sweep kernel (hadi_sweep_resident, csrc/hadi_k_resident.h) under the wave emulator: the
whole time loop of 1 - 3 instances in one launch, against the oracle and against the emulator's streaming path (the row and
column kernels the resident phases are built from, at the same strip geometry).  Shapes with fewer than 8 column chunks run
the column phase with idle wavefronts, which only keep its barrier schedule -- a drift there gives wrong fields, not a hang."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_resident.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
R_F = 0.01  # (strips need r_d != r_f)


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_resident.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", EMU_SO,
                               os.path.join(HERE, "emu", "emu_resident.cpp")])
    lib = C.CDLL(EMU_SO)
    lib.emu_set_tuning(b"reset", 0)
    return lib


def _solve(emu, m1, m2, N, strikes, Ns=None, dts=None):
    n = len(strikes)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (n, 1)).copy()
    Ni = None if Ns is None else np.array(Ns, dtype=np.int32)
    dti = None if dts is None else np.array(dts, dtype=np.float64)
    args = (C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(R_F), _P(par))
    # resident launch
    Ur = U0.copy()
    P = C.c_int(0)
    rc = emu.emu_solve_resident(n, m1, m2, N, *args, _P(vs), _P(vv), _P(ds), _P(dv), _P(Ur), 64,
                                None if Ni is None else Ni.ctypes.data_as(_ip), _P(dti), C.byref(P))
    assert rc == 0, rc
    # streaming kernels at the same geometry (one strip block per instance)
    Us = U0.copy()
    emu.emu_set_tuning(b"strip", 1)
    emu.emu_set_tuning(b"strip_blocks", 1)
    try:
        rc = emu.emu_solve(n, m1, m2, N, *args, O.EU, _P(vs), _P(vv), _P(ds), _P(dv), _P(Us), _P(U0), None,
                           8 * 256, 0, None, None, None, 64, 0, 0, None,
                           None if Ni is None else Ni.ctypes.data_as(_ip), _P(dti))
    finally:
        emu.emu_set_tuning(b"reset", 0)
    assert rc == 0, rc
    return vs, vv, ds, dv, U0, Ur, Us, P.value


def _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts):
    assert np.abs(Ur - Us).max() <= 1e-13 * np.abs(Us).max()
    for k in range(len(Ns)):
        p = O.make_params(m1, m2, Ns[k], dts[k], Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
        Uo, _, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k])
        assert np.abs(Ur[k] - Uo).max() <= 1e-10 * np.abs(Uo).max(), k


@pytest.mark.parametrize("m1,m2,N,strikes,P", [
    (300, 20, 3, [100.0], 1),            # one chunk: no reduced system, no barrier inside the column phase
    (300, 80, 3, [90.0, 110.0], 3),      # three chunks, five idle wavefronts in the column phase
    (400, 150, 2, [95.0, 105.0, 100.0], 5),
    (512, 256, 2, [100.0], 8),           # the benchmarked grid: every wavefront owns a chunk
])
def test_resident_sweep_against_oracle_and_streaming_path(emu, m1, m2, N, strikes, P):
    vs, vv, ds, dv, U0, Ur, Us, p_chunks = _solve(emu, m1, m2, N, strikes)
    assert p_chunks == P
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [N] * len(strikes), [Cm.T / N] * len(strikes))


def test_resident_sweep_per_instance_maturities(emu):
    """Every block loops to its own N_i with its own dt_i."""
    m1, m2 = 300, 80
    Ns, Ts = [3, 1, 2], [0.5, 0.2, 1.0]
    dts = [t / s for t, s in zip(Ts, Ns)]
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, 1, [90.0, 100.0, 110.0], Ns, dts)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts)
