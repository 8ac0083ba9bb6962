"""CPU-only check of the maturity ladder of the four whole-loop kernels (hadi_small_kernel, hadi_small_seq_kernel,
hadi_small_seq2_kernel, hadi_small_sch_kernel) under the wave emulator.  The product's setup, pack and locate kernels build the
inputs (tests/emu/emu_ladder.cpp).  Every snapshot is compared
  - bit for bit with the same emulated kernel run to N = snap_steps[q] (the ladder's definition), and
  - with the oracle at that N at the bound of the scheme tests, |diff| <= 1e-10 max|U_ref|, on well-conditioned grids (asserted).
Calls run with r_f = 0 (the canonical rate): the call's boundary tables carry exp(-r_f dt (N - 1)), so only then -- and for puts
-- is the state after step n the n-step solve (tests/test_oracle_ladder.py)."""
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
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_ladder.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH = range(5)
KIND_NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch"}
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
R_F = 0.0


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_ladder.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", EMU_SO,
                               os.path.join(HERE, "emu", "emu_ladder.cpp")])
    lib = C.CDLL(EMU_SO)
    lib.emu_set_tuning(b"reset", 0)
    return lib


_GRIDS = {}


def _grids(m1, m2, n):
    """Well-conditioned batch (asserted), built once per shape and left unchanged."""
    key = (m1, m2, n)
    if key not in _GRIDS:
        strikes = Cm.well_conditioned_strikes(m1, n)
        g = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
        Cm.assert_well_conditioned(g[2], g[3])
        _GRIDS[key] = (strikes,) + g
    return _GRIDS[key]


def _run(emu, m1, m2, g, kind, N, dts, snaps, variant=0, scheme=0, theta=Cm.THETA, put=False, divs=None, r_f=R_F, V0=None):
    strikes, vs, vv, ds, dv, U0 = g
    n = len(strikes)
    par8 = np.zeros((n, 8))
    for k in range(n):
        par8[k] = list(MODEL) + [dts[k], N, strikes[k] if put else 0.0, 1.0 if put else 0.0]
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    snaps = np.ascontiguousarray(snaps, dtype=np.int32)
    out = np.full((n, len(snaps)), np.nan)
    Uout = np.zeros_like(Uin)
    status = np.full(n, -1, dtype=np.int32)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in divs] if divs else [None] * 3
    rc = emu.emu_ladder(n, m1, m2, C.c_double(theta), C.c_double(Cm.R_D), C.c_double(r_f), _P(par8), _P(vs), _P(vv), _P(ds), _P(dv),
                        _P(Uin), _P(Uin), kind, variant, scheme, len(dd[0]) if divs else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]),
                        C.c_double(Cm.S_0), C.c_double(Cm.v0_for(m2) if V0 is None else V0), len(snaps), snaps.ctypes.data_as(_ip),
                        _P(out), _P(Uout), status.ctypes.data_as(_ip))
    assert rc == 0, rc
    return out, Uout, status, Uin


def _oracle_node(m1, m2, g, k, N, dt, variant, scheme, theta, put, divs, Uin, r_f=R_F):
    strikes, vs, vv, ds, dv, _ = g
    ovar = {0: O.EU, 1: O.AM, 2: O.DIV, 3: O.AM_DIV}[variant]
    if scheme:
        p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, r_f, *MODEL, O.EU)
        U = S.solve_one(p, vs[k], vv[k], ds[k], dv[k], Uin[k], {1: S.CS, 2: S.MCS, 3: S.HV}[scheme])
    else:
        p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, r_f, *MODEL, ovar, divs if variant & 2 else None,
                          option_type=O.PUT if put else O.CALL, strikes=strikes[k] if put else None)
        U = O.solve(p, vs[k], vv[k], ds[k], dv[k], Uin[k], Uin[k] if variant & 1 else None)[0]
    i0, j0 = O.find_s_index(vs[k], Cm.S_0), O.find_v_index(vv[k], Cm.v0_for(m2))
    assert i0 >= 0
    return U[i0 + j0 * (m1 + 1)], np.abs(U).max()


_SINGLE, _REF = {}, {}  # computed once, shared by the step sets of a case


def _check(emu, m1, m2, n, kind, N, snaps, dts=None, **kw):
    g = _grids(m1, m2, n)
    dts = dts or [Cm.T / N] * n
    ckey = (m1, m2, n, tuple(dts), repr(sorted(kw.items())))
    out, Uout, status, Uin = _run(emu, m1, m2, g, kind, N, dts, snaps, **kw)
    assert (status == 0).all()
    okw = {k: kw.get(k, d) for k, d in (("variant", 0), ("scheme", 0), ("theta", Cm.THETA), ("put", False), ("divs", None))}
    worst = 0.0
    for q, nq in enumerate(snaps):
        # the definition: the same emulated kernel run to N = snap_steps[q]
        if (kind, nq) + ckey not in _SINGLE:
            _SINGLE[(kind, nq) + ckey] = _run(emu, m1, m2, g, kind, nq, dts, [nq], **kw)[0]
        single = _SINGLE[(kind, nq) + ckey]
        assert np.array_equal(out[:, q], single[:, 0]), (KIND_NAMES[kind], m1, m2, nq, out[:, q] - single[:, 0])
        for k in range(n):
            if (k, nq) + ckey not in _REF:
                _REF[(k, nq) + ckey] = _oracle_node(m1, m2, g, k, nq, dts[k], Uin=Uin, **okw)
            ref, scale = _REF[(k, nq) + ckey]
            worst = max(worst, abs(out[k, q] - ref) / scale)
            assert abs(out[k, q] - ref) <= 1e-10 * scale, (KIND_NAMES[kind], m1, m2, nq, k, out[k, q], ref)
    # the snapshot of the last step is the node of the field the kernel leaves behind
    if snaps[-1] == N:
        strikes, vs, vv = g[0], g[1], g[2]
        for k in range(n):
            i0, j0 = O.find_s_index(vs[k], Cm.S_0), O.find_v_index(vv[k], Cm.v0_for(m2))
            assert out[k, -1] == Uout[k, i0 + j0 * (m1 + 1)]
    print("%s %dx%d x%d N %d snaps %s: worst |diff| / max|U| %.2e" % (KIND_NAMES[kind], m1, m2, n, N, list(snaps), worst))
    return out


def _step_sets(N):
    return [[1, N], [2, 5, N - 1], list(range(1, N + 1))]


# 8x4 the smallest; 50x25 the calibration grid; 65x16 two nodes per lane; 128x32 the largest grid hadi_small_sch_kernel admits;
# 20x30 m2 > m1 (two b1 entries on one v-row).  Three instances: the pairs kernel's odd last instance.
SHAPES = [(8, 4), (50, 25), (65, 16), (128, 32), (20, 30)]
N_STEPS = 7


# (the Douglas whole-loop kernels admit grids of up to 76 KiB of LDS: 128x32 is beyond them and runs the streaming kernels in the
# library; 100x25 is close to that limit)
DOUGLAS_CASES = [(m1, m2, k) for m1, m2 in [s if s != (128, 32) else (100, 25) for s in SHAPES] for k in (BLOCK4, BLOCK8, SEQ, SEQ2)]


@pytest.mark.parametrize("m1,m2,kind", DOUGLAS_CASES, ids=["%dx%d-%s" % (c[0], c[1], KIND_NAMES[c[2]]) for c in DOUGLAS_CASES])
def test_douglas_kernels_every_step_set(emu, m1, m2, kind):
    for snaps in _step_sets(N_STEPS):
        _check(emu, m1, m2, 3, kind, N_STEPS, snaps)


@pytest.mark.parametrize("scheme,theta", [(1, 0.5), (2, TH_MCS), (3, TH_HV)], ids=["CS", "MCS", "HV"])
@pytest.mark.parametrize("m1,m2", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_scheme_kernel_every_step_set(emu, m1, m2, scheme, theta):
    for snaps in _step_sets(N_STEPS):
        _check(emu, m1, m2, 2, SCH, N_STEPS, snaps, scheme=scheme, theta=theta)


def _paying_steps(emu, N, dt):
    dates = np.ascontiguousarray(Cm.DIVS[0], dtype=np.float64)
    flags = np.full(N, -1, dtype=np.int32)
    emu.emu_dividend_steps(N, C.c_double(dt), len(dates), _P(dates), flags.ctypes.data_as(_ip), N)
    return [q + 1 for q in range(N) if flags[q] >= 0]


@pytest.mark.parametrize("kind", [BLOCK4, SEQ, SEQ2])
def test_dividends_with_snapshots_on_paying_steps(emu, kind):
    N = 10
    pay = _paying_steps(emu, N, Cm.T / N)
    assert len(pay) >= 2
    snaps = sorted(set(pay + [p + 1 for p in pay if p + 1 <= N] + [1]))  # every paying step and the step after it
    _check(emu, 50, 25, 3, kind, N, snaps, variant=2, divs=Cm.DIVS)


@pytest.mark.parametrize("kind", [BLOCK4, BLOCK8])
@pytest.mark.parametrize("variant", [1, 3], ids=["AM", "AM_DIV"])
def test_american(emu, kind, variant):
    N = 10
    pay = _paying_steps(emu, N, Cm.T / N)
    _check(emu, 50, 25, 2, kind, N, sorted(set([1, 4, N] + pay[:1])), variant=variant, divs=Cm.DIVS if variant & 2 else None)


@pytest.mark.parametrize("kind", [BLOCK4, SEQ, SEQ2])
def test_puts(emu, kind):
    _check(emu, 50, 25, 3, kind, 6, [1, 3, 6], put=True)


@pytest.mark.parametrize("kind", [BLOCK8, SEQ, SEQ2, SCH])
def test_per_instance_delta_t(emu, kind):
    """Every instance its own ladder in time on the shared step indices."""
    kw = {"scheme": 2, "theta": TH_MCS} if kind == SCH else {}
    _check(emu, 50, 25, 3, kind, 6, [2, 3, 6], dts=[Cm.T / 6, 0.5 / 6, 0.25 / 6], **kw)


def test_off_grid_spot_is_reported_and_written_as_nan(emu):
    g = _grids(50, 25, 3)
    strikes, vs, vv, ds, dv, U0 = g
    par8 = np.array([list(MODEL) + [Cm.T / 4, 4, 0.0, 0.0]] * 3)
    snaps = np.array([2, 4], dtype=np.int32)
    out = np.zeros((3, 2))
    status = np.zeros(3, dtype=np.int32)
    rc = emu.emu_ladder(3, 50, 25, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(R_F), _P(par8), _P(vs), _P(vv), _P(ds), _P(dv),
                        _P(U0), None, SEQ2, 0, 0, 0, None, None, None, C.c_double(Cm.S_0 + 0.123), C.c_double(Cm.V_0), 2,
                        snaps.ctypes.data_as(_ip), _P(out), None, status.ctypes.data_as(_ip))
    assert rc == 0 and (status == 1).all() and np.isnan(out).all()


def test_a_call_without_snapshots_is_untouched(emu):
    """n_snap = 0 (every call but the ladder's): the field is that of the ladder run, nothing is written to the output."""
    g = _grids(50, 25, 3)
    _, U_lad, _, _ = _run(emu, 50, 25, g, SEQ, 5, [Cm.T / 5] * 3, [1, 5])
    strikes, vs, vv, ds, dv, U0 = g
    par8 = np.array([list(MODEL) + [Cm.T / 5, 5, 0.0, 0.0]] * 3)
    Uout = np.zeros_like(U0)
    status = np.zeros(3, dtype=np.int32)
    rc = emu.emu_ladder(3, 50, 25, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(R_F), _P(par8), _P(vs), _P(vv), _P(ds), _P(dv),
                        _P(U0), None, SEQ, 0, 0, 0, None, None, None, C.c_double(Cm.S_0), C.c_double(Cm.V_0), 0, None, None, _P(Uout),
                        status.ctypes.data_as(_ip))
    assert rc == 0 and np.array_equal(Uout, U_lad)
