"""CPU-only check of the resident sweep kernel (hadi_sweep_resident, csrc/hadi_k_resident.h) under the wave emulator: the
whole time loop of 1 - 3 instances in one launch, against the oracle and against the emulator's streaming path (the row and
column kernels the resident phases are built from, at the same strip geometry).  Shapes with fewer than 8 column chunks run
the column phase with idle wavefronts, which only keep its barrier schedule -- a drift there gives wrong fields, not a hang.

The cases added with the admitted-domain sweep (every chunk count 1 .. 8, strips of 1 .. 33 rows with a short, one-row or
empty partner strip, wavefronts without a strip, per-instance model parameters and maturities, put boundary data, theta = 1,
a 12-step loop and a recorded random sweep) run on WELL-CONDITIONED grids only and assert it (Cm.assert_well_conditioned,
the 30x rule of DESIGN.md section 2): the 1e-10 bound against the oracle belongs to such grids."""
import ctypes as C
import os
import random
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


def _solve(emu, m1, m2, N, strikes, Ns=None, dts=None, par=None, put=False, theta=Cm.THETA, V0=Cm.V_0):
    """par: per-instance rows (rho, sigma, kappa, eta), [n][4] (None: the canonical set for every instance); put: put payoff
    and put boundary data."""
    n = len(strikes)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes, V0)
    if put:
        U0 = Cm.put_payoff(vs, strikes, m2)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (n, 1)) if par is None else np.asarray(par, dtype=np.float64)
    par = np.ascontiguousarray(par).reshape(n, 4).copy()
    ks = np.ascontiguousarray(strikes, dtype=np.float64)
    Ni = None if Ns is None else np.array(Ns, dtype=np.int32)
    dti = None if dts is None else np.array(dts, dtype=np.float64)
    args = (C.c_double(Cm.T / N), C.c_double(theta), C.c_double(Cm.R_D), C.c_double(R_F), _P(par))
    # resident launch
    Ur = U0.copy()
    P = C.c_int(0)
    rc = emu.emu_solve_resident(n, m1, m2, N, *args, _P(vs), _P(vv), _P(ds), _P(dv), _P(Ur), 64,
                                None if Ni is None else Ni.ctypes.data_as(_ip), _P(dti), C.byref(P), _P(ks), 1 if put else 0)
    assert rc == 0, rc
    # streaming kernels at the same geometry (one strip block per instance)
    Us = U0.copy()
    emu.emu_set_tuning(b"strip", 1)
    emu.emu_set_tuning(b"strip_blocks", 1)
    try:
        rc = emu.emu_solve(n, m1, m2, N, *args, O.EU, _P(vs), _P(vv), _P(ds), _P(dv), _P(Us), _P(U0), None,
                           8 * 256, 0, None, None, None, 64, 0, 0, _P(ks) if put else None,
                           None if Ni is None else Ni.ctypes.data_as(_ip), _P(dti))
    finally:
        emu.emu_set_tuning(b"reset", 0)
    assert rc == 0, rc
    return vs, vv, ds, dv, U0, Ur, Us, P.value


def _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts, par=None, put=False, theta=Cm.THETA, strikes=None):
    rel = np.abs(Ur - Us).max() / np.abs(Us).max()
    worst = 0.0
    for k in range(len(Ns)):
        model = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA) if par is None else tuple(par[k])
        p = O.make_params(m1, m2, Ns[k], dts[k], theta, Cm.R_D, R_F, *model, O.EU,
                          option_type=O.PUT if put else O.CALL, strikes=[strikes[k]] if put else None)
        Uo, _, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k])
        worst = max(worst, np.abs(Ur[k] - Uo).max() / np.abs(Uo).max())
    print("resident vs streaming %.3e, vs oracle %.3e" % (rel, worst))
    assert rel <= 1e-13
    assert worst <= 1e-10


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


# ---- the admitted domain: chunk counts, strip edges, inputs (well-conditioned grids, asserted) -------------------------------

def _strip_rows(m2):
    """Rows of the eight strips of one block per instance: height ceil(rows / 8); the last strips are short or empty."""
    rows = m2 + 1
    rs = (rows + 7) // 8
    return rs, [max(0, min(rs, rows - w * rs)) for w in range(8)]


@pytest.mark.parametrize("m1,m2,P,rs,last", [
    # m2 + 1 rows as 8 strips of rs rows: what the LAST non-empty strip and the wavefronts behind it look like
    (300, 3, 1, 1, "4 strips of 1 row, 4 wavefronts without a strip"),
    (300, 9, 1, 2, "5 strips of 2 rows, 3 wavefronts without a strip"),
    (300, 32, 1, 5, "6 strips of 5 rows, a last strip of 3, one wavefront without a strip"),
    (300, 33, 2, 5, "6 strips of 5 rows, a last strip of 4, one wavefront without a strip"),
    (300, 56, 2, 8, "7 strips of 8 rows and a last strip of ONE row"),
    (300, 57, 2, 8, "7 strips of 8 rows and a last strip of 2"),
    (300, 65, 2, 9, "7 strips of 9 rows and a last strip of 3"),
    (300, 131, 4, 17, "7 strips of 17 rows and a last strip of 13"),
    (300, 197, 6, 25, "7 strips of 25 rows and a last strip of 23"),
    (300, 230, 7, 29, "7 strips of 29 rows and a last strip of 28"),
    (300, 263, 8, 33, "8 full strips of 33 rows"),
    (257, 67, 3, 9, "the narrowest 8-nodes-per-lane row"),
    (512, 67, 3, 9, "the widest"),
])
def test_resident_sweep_chunk_counts_and_strip_edges(emu, m1, m2, P, rs, last):
    """One instance, two steps (the second runs on the state, the LDS and the barrier phase the first left behind): P = 1, 2,
    4, 6, 7, 8 column chunks -- idle wavefronts in the column phase -- and strips whose partner is short, one row long, empty
    or absent altogether."""
    assert (_strip_rows(m2)[0], (m2 + 1 + 32) // 33) == (rs, P)
    V0 = Cm.v0_for(m2)
    vs, vv, ds, dv, U0, Ur, Us, p_chunks = _solve(emu, m1, m2, 2, [100.0], V0=V0)
    Cm.assert_well_conditioned(ds, dv)
    assert p_chunks == P
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [2], [Cm.T / 2])


def test_strip_edge_list_covers_the_edge_kinds():
    """The parameter list above really holds the edges it names (so that a change of the list cannot hollow it out)."""
    geo = {m2: _strip_rows(m2)[1] for m2 in (3, 9, 32, 33, 56, 57, 65, 131, 197, 230, 263)}
    assert geo[3] == [1, 1, 1, 1, 0, 0, 0, 0] and geo[9] == [2] * 5 + [0] * 3    # wavefronts without a strip
    assert geo[56] == [8] * 7 + [1] and geo[57] == [8] * 7 + [2]                  # a last strip of one row / of two
    assert geo[32][-2:] == [3, 0] and geo[33][-2:] == [4, 0]                      # a short strip whose partner is empty
    assert geo[263] == [33] * 8 and geo[131][-1] == 13 and geo[230][-1] == 28
    assert sorted({(m2 + 33) // 33 for m2 in geo}) == [1, 2, 4, 6, 7, 8]


PER_INSTANCE_PAR = [(-0.9, 0.3, 1.5, 0.04), (0.0, 0.7, 0.5, 0.15), (0.3, 0.15, 3.5, 0.02)]


def test_resident_sweep_per_instance_parameters_and_maturities(emu):
    """Three instances with their own (rho, sigma, kappa, eta), strike, N_i and dt_i: every table (s-coefficients, row
    constants, the column phase's a.pb / a.rinv) and every a.ipar entry must be the instance's own.  Instance 0 is NOT the
    longest, so a block that took instance 0's tables or step count shows against the oracle."""
    m1, m2 = 300, 80
    strikes = Cm.well_conditioned_strikes(m1, 3)
    Ns, Ts = [2, 3, 1], [0.7, 0.4, 1.1]
    dts = [t / s for t, s in zip(Ts, Ns)]
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, 1, strikes, Ns, dts, par=PER_INSTANCE_PAR)
    Cm.assert_well_conditioned(ds, dv)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts, par=PER_INSTANCE_PAR)


def test_resident_sweep_put_boundary_data(emu):
    """Put payoff with the put boundary data (par8[6] = K, par8[7] = 1: the row constants' boundary values K e^{-r_d t})."""
    m1, m2, N = 300, 80, 2
    strikes = [100.0, 92.5]
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, N, strikes, put=True)
    Cm.assert_well_conditioned(ds, dv)
    assert np.abs(Ur - Us).max() <= 1e-13 * np.abs(Us).max()
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=R_F, option_type=O.PUT, strikes=np.array(strikes))
    Uo, _, _ = O.solve_batch(p, vs, vv, ds, dv, U0)
    err = np.abs(Ur - Uo).max() / np.abs(Uo).max()
    print("put data: vs oracle %.3e" % err)
    assert err <= 1e-10
    pc = Cm.oracle_params(m1, m2, N, "EU", r_f=R_F)  # (the data matter: the call boundary on the same payoff is another field)
    Uc, _, _ = O.solve_batch(pc, vs, vv, ds, dv, U0)
    assert np.abs(Uc - Uo).max() > 1e-6 * np.abs(Uo).max()


def test_resident_sweep_theta_one(emu):
    """theta = 1: the strips' (1 - theta) / theta scale of the explicit A1 action is exactly 0."""
    m1, m2, N = 300, 80, 2
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, N, [100.0], theta=1.0)
    Cm.assert_well_conditioned(ds, dv)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [N], [Cm.T / N], theta=1.0)


def test_resident_sweep_twelve_steps(emu):
    """Twelve steps in one launch: the column phase's LDS aliases the next step's ring prologue eleven times over."""
    m1, m2, N = 300, 20, 12
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, N, [100.0])
    Cm.assert_well_conditioned(ds, dv)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [N], [Cm.T / N])


# ---- a recorded random sweep of eligible problems ----------------------------------------------------------------------
RANDOM_SEED = 20260
RANDOM_CASES = [  # (m1, m2, put, theta, strikes, [(rho, sigma, kappa, eta)], maturities): _draw_random_cases(RANDOM_SEED), written out as a record
    (387, 91, True, 1.0, [109.0297], [(-0.679, 0.2092, 2.4738, 0.0101)], [0.249]),
    (486, 21, True, 0.07, [97.7458, 111.4743], [(-0.5783, 0.7257, 2.1248, 0.0313), (-0.9053, 0.7725, 1.8139, 0.0851)], [0.763, 0.928]),
    (289, 60, False, 0.5, [114.1462, 87.3141], [(0.4605, 0.6094, 0.4248, 0.0906), (0.1848, 0.7095, 3.3665, 0.0344)], [0.854, 1.237]),
    (442, 77, False, 0.793, [94.117], [(-0.37, 0.3593, 1.212, 0.0923)], [0.927]),
    (335, 64, False, 0.65, [89.2987], [(-0.4788, 0.2608, 3.8569, 0.1271)], [0.664]),
    (325, 130, False, 0.128, [94.2787], [(-0.7803, 0.3961, 1.2308, 0.0274)], [1.461]),
    (364, 24, True, 0.679, [91.1272, 114.4016], [(-0.7932, 0.3475, 0.4638, 0.1233), (0.2894, 0.727, 0.978, 0.1909)], [0.361, 1.071]),
    (495, 51, False, 0.65, [110.9277, 88.1181], [(-0.8851, 0.3127, 3.7279, 0.1605), (0.4106, 0.7519, 3.8199, 0.1944)], [0.397, 0.798]),
    (468, 141, True, 0.5, [106.3988], [(-0.7666, 0.2923, 1.4037, 0.1153)], [0.96]),
    (359, 4, False, 0.944, [108.0129, 103.6844], [(-0.2048, 0.6063, 1.2845, 0.1387), (-0.8571, 0.6849, 2.1515, 0.1979)], [1.267, 0.248]),
    (482, 62, False, 1.0, [112.1265], [(-0.3131, 0.2073, 3.6399, 0.0774)], [0.393]),
    (340, 64, True, 0.5, [104.4414, 88.278], [(0.1575, 0.768, 3.9863, 0.0867), (-0.8709, 0.691, 3.5222, 0.0896)], [0.22, 0.675]),
]


def _draw_random_cases(seed, count=12):
    """A generator of its own (not the one behind test_random_shapes_and_kernel_choices_vs_oracle, whose seeds are a record):
    m1 in 257 .. 512, m2 in 3 .. 263, one or two instances, N = 2, rows x steps x instances <= 300 (the emulator's cost),
    call or put, theta in (0, 1], per-instance strikes, model parameters (the ranges of tools/gpu_sweep.py) and maturities.
    Draws whose s- or v-grid breaks the 30x rule are drawn again."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        m1, m2, n = rng.randint(257, 512), rng.randint(3, 263), rng.randint(1, 2)
        put = rng.random() < 0.5
        theta = rng.choice([0.5, 1.0]) if rng.random() < 0.4 else round(rng.uniform(0.05, 1.0), 3)
        strikes = [round(rng.uniform(85, 115), 4) for _ in range(n)]
        par = [(round(rng.uniform(-0.95, 0.5), 4), round(rng.uniform(0.1, 0.8), 4), round(rng.uniform(0.3, 4.0), 4),
                round(rng.uniform(0.01, 0.2), 4)) for _ in range(n)]
        Ts = [round(rng.uniform(0.2, 1.5), 3) for _ in range(n)]
        if (m2 + 1) * 2 * n > 300:
            continue
        _, _, ds, dv, _ = Cm.oracle_grids(m1, m2, strikes)
        if Cm.interval_ratios(ds).max() > Cm.COND_MAX or Cm.interval_ratios(dv).max() > Cm.COND_MAX:
            continue
        out.append((m1, m2, put, theta, strikes, par, Ts))
    return out


def test_random_case_list_is_the_record_of_its_seed():
    assert _draw_random_cases(RANDOM_SEED) == RANDOM_CASES


@pytest.mark.parametrize("m1,m2,put,theta,strikes,par,Ts", RANDOM_CASES,
                         ids=["%dx%d_%s_n%d" % (c[0], c[1], "put" if c[2] else "call", len(c[4])) for c in RANDOM_CASES])
def test_resident_sweep_random_eligible_problems(emu, m1, m2, put, theta, strikes, par, Ts):
    N = 2
    Ns, dts = [N] * len(strikes), [t / N for t in Ts]
    vs, vv, ds, dv, U0, Ur, Us, P = _solve(emu, m1, m2, 1, strikes, Ns, dts, par=par, put=put, theta=theta)
    Cm.assert_well_conditioned(ds, dv)
    assert P == (m2 + 33) // 33
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts, par=par, put=put, theta=theta, strikes=strikes)
