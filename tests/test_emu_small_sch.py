"""CPU-only check of hadi_small_sch_kernel (csrc/hadi_k_small_sch.h: the whole time loop of Craig-Sneyd, Modified Craig-Sneyd
and Hundsdorfer-Verwer sweeps in LDS, one wavefront per instance) under the wave emulator.  The product's setup and pack kernels
build the tables and the packed state; the full field is compared with the restatement tests/scheme_ref.py at the project's
bound for scheme kernels, 1e-10 max|U_ref| (tests/test_gpu_schemes.py), on well-conditioned grids (asserted)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import scheme_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_small_sch.so")
_dp = C.POINTER(C.c_double)

TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(S.CS, 0.5, "CS"), (S.MCS, TH_MCS, "MCS"), (S.HV, TH_HV, "HV")]
R_F = 0.007
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)


def _P(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", EMU_SO,
                               os.path.join(HERE, "emu", "emu_small_sch.cpp")])
    lib = C.CDLL(EMU_SO)
    lib.emu_set_tuning(b"reset", 0)
    return lib


def _grids(m1, m2, n):
    strikes = Cm.well_conditioned_strikes(m1, n)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    return vs, vv, ds, dv, U0


def _emu_run(emu, m1, m2, grids, scheme, theta, r_f, models, Ns, dts):
    vs, vv, ds, dv, U0 = grids
    n = len(Ns)
    par8 = np.zeros((n, 8))
    for k in range(n):
        par8[k] = list(models[k]) + [dts[k], Ns[k], 0.0, 0.0]
    U = np.ascontiguousarray(U0.copy())
    lds = C.c_longlong(0)
    rc = emu.emu_small_sch(n, m1, m2, C.c_double(theta), C.c_double(Cm.R_D), C.c_double(r_f), _P(par8), _P(vs), _P(vv), _P(ds),
                           _P(dv), _P(U), scheme, 64, C.byref(lds))
    assert rc == 0, rc
    return U, lds.value


def _ref_one(m1, m2, grids, k, scheme, theta, r_f, model, N, dt):
    vs, vv, ds, dv, U0 = grids
    p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, r_f, *model, O.EU)
    return S.solve_one(p, vs[k], vv[k], ds[k], dv[k], U0[k], scheme)


def _check(emu, m1, m2, scheme, theta, N, n=2, r_f=R_F):
    grids = _grids(m1, m2, n)
    U, lds = _emu_run(emu, m1, m2, grids, scheme, theta, r_f, [MODEL] * n, [N] * n, [Cm.T / N] * n)
    worst = 0.0
    for k in range(n):
        Uo = _ref_one(m1, m2, grids, k, scheme, theta, r_f, MODEL, N, Cm.T / N)
        rel = np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        worst = max(worst, rel)
        assert rel <= 1e-10, (m1, m2, scheme, k, rel)
    print("%dx%d scheme %d theta %.4f N %d r_f %g: %d B of LDS, worst |diff| / max|U| %.2e" % (m1, m2, scheme, theta, N, r_f, lds, worst))
    return U, lds


# 8x4 the smallest; 50x25 one node per lane; 51x7 / 52x8 / 53x31 the m1 mod 4 remainders of the four-node rounds and 8 / 9 / 32
# v-rows for the eight-row rounds of the column sweep; 20x30 m2 > m1 (two b1 entries on one v-row); 64x32 / 65x16 the one / two
# nodes-per-lane boundary, 33 v-rows; 100x20 two nodes per lane; 128x32 the largest admitted grid
SHAPES = [(8, 4, 2), (50, 25, 3), (51, 7, 2), (52, 8, 4), (53, 31, 3), (20, 30, 2), (64, 32, 3), (65, 16, 4), (100, 20, 2), (128, 32, 2)]


@pytest.mark.parametrize("scheme,theta,name", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_full_field_vs_restatement(emu, m1, m2, N, scheme, theta, name):
    _, lds = _check(emu, m1, m2, scheme, theta, N)
    pitch = (m1 + 3) | 1
    assert 4 * (m2 + 1) * pitch * 8 < lds <= 160 * 1024  # four fields and the tables, within a CU's LDS


def test_layout_sizes_of_the_design_note(emu):
    """DESIGN.md section 4.1 quotes them: 50x25 three instances per CU, 128x32 one."""
    lds = {}
    for m1, m2 in ((50, 25), (128, 32)):
        grids = _grids(m1, m2, 1)
        lds[m1] = _emu_run(emu, m1, m2, grids, S.CS, 0.5, R_F, [MODEL], [1], [Cm.T])[1]
    assert 3 * lds[50] <= 160 * 1024 < 4 * lds[50]
    assert lds[128] <= 160 * 1024 < 2 * lds[128]


@pytest.mark.parametrize("scheme,theta,N,r_f", [(S.MCS, TH_MCS, 3, 0.0), (S.HV, TH_HV, 3, Cm.R_D), (S.MCS, 1.0, 3, R_F), (S.HV, 1.0, 3, R_F),
                                                (S.CS, 1.0, 3, R_F), (S.MCS, 0.75, 3, R_F), (S.CS, 0.0, 1, R_F)],
                         ids=["rf0", "rf_eq_rd", "MCS_theta1", "HV_theta1", "CS_theta1", "MCS_theta075", "CS_explicit"])
def test_rates_and_thetas(emu, scheme, theta, N, r_f):
    """(Explicit Craig-Sneyd takes one step: more steps of this size grow without bound, and the round-off with them.)"""
    _check(emu, 50, 25, scheme, theta, N, r_f=r_f)


@pytest.mark.parametrize("scheme,theta,name", SCHEMES, ids=[s[2] for s in SCHEMES])
def test_per_instance_parameters_and_maturities(emu, scheme, theta, name):
    """Four instances with their own rho, sigma, kappa, eta and (N_i, dt_i): each stops at its own N (dispatched longest first)
    and takes dt, theta dt, e_n and the scheme's constants from its own instance."""
    m1, m2 = 50, 25
    models = [(-0.9, 0.3, 1.5, 0.04), (-0.5, 0.5, 2.0, 0.09), (0.0, 0.2, 0.5, 0.02), (0.3, 0.4, 3.0, 0.06)]
    Ts, Ns = [0.5, 1.0, 0.8, 0.25], [5, 8, 3, 1]
    dts = [t / s for t, s in zip(Ts, Ns)]
    grids = _grids(m1, m2, 4)
    U, _ = _emu_run(emu, m1, m2, grids, scheme, theta, R_F, models, Ns, dts)
    for k in range(4):
        Uo = _ref_one(m1, m2, grids, k, scheme, theta, R_F, models[k], Ns[k], dts[k])
        assert np.abs(U[k] - Uo).max() <= 1e-10 * np.abs(Uo).max(), k


@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)])
def test_mcs_at_one_half_is_craig_sneyd(emu, m1, m2):
    grids = _grids(m1, m2, 2)
    args = (R_F, [MODEL] * 2, [4] * 2, [Cm.T / 4] * 2)
    U, _ = _emu_run(emu, m1, m2, grids, S.MCS, 0.5, *args)
    Uc, _ = _emu_run(emu, m1, m2, grids, S.CS, 0.5, *args)
    assert np.abs(U - Uc).max() <= 1e-12 * np.abs(Uc).max()


def test_refuses_what_the_kernel_does_not_cover(emu):
    vs, vv, ds, dv, U0 = _grids(129, 32, 1)  # m1 > 128: not admitted
    par8 = np.array([list(MODEL) + [Cm.T, 1, 0.0, 0.0]])
    U = U0.copy()

    def call(m1, m2, scheme, theta, g):
        return emu.emu_small_sch(1, m1, m2, C.c_double(theta), C.c_double(Cm.R_D), C.c_double(R_F), _P(par8), _P(g[0]), _P(g[1]),
                                 _P(g[2]), _P(g[3]), _P(U), scheme, 64, None)

    assert call(129, 32, 1, 0.5, (vs, vv, ds, dv)) == 3
    g = _grids(50, 33, 1)  # m2 > 32
    U = g[4].copy()
    assert call(50, 33, 1, 0.5, g) == 3
    g = _grids(50, 25, 1)
    U = g[4].copy()
    assert call(50, 25, 0, 0.5, g) == 3 and call(50, 25, 2, 0.0, g) == 3 and call(50, 25, 3, 0.0, g) == 3
