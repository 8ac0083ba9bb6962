"""CPU-only check of the sampled ladder of the four whole-loop kernels (hadi_small_kernel, hadi_small_seq_kernel,
hadi_small_seq2_kernel, hadi_small_sch_kernel) under the wave emulator.  The product's setup, pack and sample-locate kernels build
the inputs (tests/emu/emu_samples.cpp).  Grid 50x25, five instances (the pairs kernel gets an odd last block), N = 6, snapshots
[1, 3, 6], ten spots per instance (samples_ref.kernel_test_spots: S_0, two other nodes, five interior off-node spots, one in the
first and one in the last interval).
  - The S_0 column equals the emulated ladder (emu_ladder, same kernel) bit for bit.
  - Everything is compared with samples_ref applied to oracle fields at N = snap_steps[q], at the bound
    |diff| <= 1e-10 sum|w| |scale| max|U_ref| on well-conditioned grids (asserted).
  - Off-grid spots give NaN and the flag word.
Mutations of hadi_sample_lds / hadi_sample_locate_kernel that turn this file red (tried on the emulator build only): instance 0's
taps for everyone (rows = n cases), a packed offset used as a natural one (seq / pairs / sch), the stencil not clamped at m1 - 3
(the last-interval spot), i taken as the first node >= x (every interior spot), the sample read one step late (every snapshot)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import samples_ref as R
import scheme_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_samples.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH = range(5)
KIND_NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch"}
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
M1, M2, N_INST, N_STEPS, SNAPS = 50, 25, 5, 6, [1, 3, 6]


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_samples.cpp", "emu_ladder.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", EMU_SO,
                               os.path.join(HERE, "emu", "emu_samples.cpp")])
    lib = C.CDLL(EMU_SO)
    lib.emu_set_tuning(b"reset", 0)
    return lib


_G = {}


def _grids():
    """Well-conditioned batch (asserted), built once and left unchanged; with each instance's ten spots."""
    if not _G:
        strikes = Cm.well_conditioned_strikes(M1, N_INST)
        g = Cm.oracle_grids(M1, M2, strikes, V0=Cm.v0_for(M2))
        Cm.assert_well_conditioned(g[2], g[3])
        _G["g"] = (strikes,) + g
        _G["spots"] = np.ascontiguousarray(np.stack([R.kernel_test_spots(g[0][k], Cm.S_0) for k in range(N_INST)]))
    return _G["g"], _G["spots"]


def _par8(strikes, dts, put):
    return np.array([list(MODEL) + [dts[k], N_STEPS, strikes[k] if put else 0.0, 1.0 if put else 0.0] for k in range(len(strikes))])


def _run(emu, kind, spots, scales, dts, variant=0, scheme=0, theta=Cm.THETA, put=False, divs=None):
    (strikes, vs, vv, ds, dv, U0), _ = _grids()
    n = len(strikes)
    par8 = _par8(strikes, dts, put)
    Uin = Cm.put_payoff(vs, strikes, M2) if put else U0
    spots = np.ascontiguousarray(np.atleast_2d(spots), dtype=np.float64)
    scales = None if scales is None else np.ascontiguousarray(np.atleast_2d(scales), dtype=np.float64)
    snaps = np.ascontiguousarray(SNAPS, dtype=np.int32)
    n_samp = spots.shape[1]
    out = np.full((n, len(SNAPS), n_samp), 7.0)
    flags = np.full((n, n_samp), -1, dtype=np.int32)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in divs] if divs else [None] * 3
    rc = emu.emu_samples(n, M1, M2, C.c_double(theta), C.c_double(Cm.R_D), C.c_double(0.0), _P(par8), _P(vs), _P(vv), _P(ds), _P(dv),
                         _P(Uin), _P(Uin), kind, variant, scheme, len(dd[0]) if divs else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]),
                         C.c_double(Cm.v0_for(M2)), n_samp, _P(spots), _P(scales), spots.shape[0], len(SNAPS),
                         snaps.ctypes.data_as(_ip), _P(out), flags.ctypes.data_as(_ip))
    assert rc == 0, rc
    return out, flags, Uin


def _ladder(emu, kind, dts, variant=0, scheme=0, theta=Cm.THETA, put=False, divs=None):
    """The emulated maturity ladder of the same kernel: [n][n_snap] at the node of S_0."""
    (strikes, vs, vv, ds, dv, U0), _ = _grids()
    n = len(strikes)
    par8 = _par8(strikes, dts, put)
    Uin = Cm.put_payoff(vs, strikes, M2) if put else U0
    snaps = np.ascontiguousarray(SNAPS, dtype=np.int32)
    out = np.full((n, len(SNAPS)), np.nan)
    status = np.full(n, -1, dtype=np.int32)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in divs] if divs else [None] * 3
    rc = emu.emu_ladder(n, M1, M2, C.c_double(theta), C.c_double(Cm.R_D), C.c_double(0.0), _P(par8), _P(vs), _P(vv), _P(ds), _P(dv),
                        _P(Uin), _P(Uin), kind, variant, scheme, len(dd[0]) if divs else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]),
                        C.c_double(Cm.S_0), C.c_double(Cm.v0_for(M2)), len(SNAPS), snaps.ctypes.data_as(_ip), _P(out), None,
                        status.ctypes.data_as(_ip))
    assert rc == 0 and (status == 0).all()
    return out


_REF = {}  # oracle fields: computed once per (problem, step), shared by the kernels of a case


def _oracle_fields(nq, dts, variant, scheme, theta, put, divs, Uin):
    key = (nq, tuple(dts), variant, scheme, theta, put, divs is not None)
    if key not in _REF:
        (strikes, vs, vv, ds, dv, _), _ = _grids()
        ovar = {0: O.EU, 1: O.AM, 2: O.DIV, 3: O.AM_DIV}[variant]
        fields = []
        for k in range(len(strikes)):
            if scheme:
                p = O.make_params(M1, M2, nq, dts[k], theta, Cm.R_D, 0.0, *MODEL, O.EU)
                fields.append(S.solve_one(p, vs[k], vv[k], ds[k], dv[k], Uin[k], {1: S.CS, 2: S.MCS, 3: S.HV}[scheme]))
            else:
                p = O.make_params(M1, M2, nq, dts[k], theta, Cm.R_D, 0.0, *MODEL, ovar, divs if variant & 2 else None,
                                  option_type=O.PUT if put else O.CALL, strikes=strikes[k] if put else None)
                fields.append(O.solve(p, vs[k], vv[k], ds[k], dv[k], Uin[k], Uin[k] if variant & 1 else None)[0])
        _REF[key] = np.stack(fields)
    return _REF[key]


def _check(emu, kind, rows_n=True, scaled=False, dts=None, **kw):
    (strikes, vs, vv, ds, dv, _), spots_n = _grids()
    n = len(strikes)
    dts = dts or [Cm.T / N_STEPS] * n
    if rows_n:
        spots = spots_n
    else:  # one list for the batch: S_0 (a node everywhere) and off-node spots inside every instance's grid
        spots = np.array([[Cm.S_0, 3.21, 61.7, 93.3, 101.9, 127.4, 250.3, 519.0, 600.0, 0.011]])
    scales = None
    if scaled:
        scales = 0.5 + 0.25 * np.arange(spots.size).reshape(spots.shape) % 7
        scales[:, 0] = 1.0  # (the S_0 column stays comparable with the ladder)
    out, flags, Uin = _run(emu, kind, spots, scales, dts, **kw)
    assert (flags == 0).all()
    # the S_0 column is the ladder, bit for bit
    assert np.array_equal(out[:, :, 0], _ladder(emu, kind, dts, **kw)), KIND_NAMES[kind]
    okw = {k: kw.get(k, d) for k, d in (("variant", 0), ("scheme", 0), ("theta", Cm.THETA), ("put", False), ("divs", None))}
    worst = 0.0
    for q, nq in enumerate(SNAPS):
        U = _oracle_fields(nq, dts, Uin=Uin, **okw)
        ref, amp, rflags = R.sample_batch(U, vs, vv, Cm.v0_for(M2), spots, scales)
        assert (rflags == 0).all()
        bound = 1e-10 * amp * np.abs(U).max(axis=1, keepdims=True)
        diff = np.abs(out[:, q, :] - ref)
        worst = max(worst, (diff / bound).max())
        assert (diff <= bound).all(), (KIND_NAMES[kind], nq, np.argwhere(diff > bound)[:4], (diff / bound).max())
    print("%s rows=%s scaled=%s %s: worst |diff| / bound %.2e" % (KIND_NAMES[kind], "n" if rows_n else "1", scaled, sorted(kw), worst))
    return out


@pytest.mark.parametrize("kind", [BLOCK4, BLOCK8, SEQ, SEQ2], ids=lambda k: KIND_NAMES[k])
@pytest.mark.parametrize("rows_n", [True, False], ids=["rows-n", "rows-1"])
def test_douglas_kernels(emu, kind, rows_n):
    _check(emu, kind, rows_n=rows_n, scaled=not rows_n)


@pytest.mark.parametrize("scheme,theta", [(1, 0.5), (2, TH_MCS), (3, TH_HV)], ids=["CS", "MCS", "HV"])
def test_scheme_kernel(emu, scheme, theta):
    _check(emu, SCH, scheme=scheme, theta=theta, scaled=True)


@pytest.mark.parametrize("kind", [BLOCK4, BLOCK8], ids=lambda k: KIND_NAMES[k])
def test_american_on_the_block_kernels(emu, kind):
    _check(emu, kind, variant=1)


def _paying_steps(emu, N, dt):
    dates = np.ascontiguousarray(Cm.DIVS[0], dtype=np.float64)
    flags = np.full(N, -1, dtype=np.int32)
    emu.emu_dividend_steps(N, C.c_double(dt), len(dates), _P(dates), flags.ctypes.data_as(_ip), N)
    return [q + 1 for q in range(N) if flags[q] >= 0]


@pytest.mark.parametrize("kind", [BLOCK4, SEQ, SEQ2], ids=lambda k: KIND_NAMES[k])
def test_dividends_with_a_snapshot_on_a_paying_step(emu, kind):
    assert set(_paying_steps(emu, N_STEPS, Cm.T / N_STEPS)) & set(SNAPS)
    _check(emu, kind, variant=2, divs=Cm.DIVS)


@pytest.mark.parametrize("kind", [BLOCK4, SEQ, SEQ2], ids=lambda k: KIND_NAMES[k])
def test_puts(emu, kind):
    _check(emu, kind, put=True, scaled=True)


@pytest.mark.parametrize("kind", [BLOCK8, SEQ, SEQ2, SCH], ids=lambda k: KIND_NAMES[k])
def test_per_instance_delta_t(emu, kind):
    kw = {"scheme": 2, "theta": TH_MCS} if kind == SCH else {}
    _check(emu, kind, dts=[Cm.T / 6, 0.5 / 6, 0.25 / 6, 0.75 / 6, 0.6 / 6], **kw)


@pytest.mark.parametrize("kind", [BLOCK4, SEQ2, SCH], ids=lambda k: KIND_NAMES[k])
def test_off_grid_spots_are_nan_and_flagged(emu, kind):
    (strikes, vs, vv, ds, dv, _), spots_n = _grids()
    spots = spots_n.copy()
    spots[1, 3] = vs[1, 0] - 1e-3       # below the grid
    spots[2, 9] = vs[2, M1] + 1e-3      # above it
    spots[4, 0] = np.nan
    kw = {"scheme": 1, "theta": 0.5} if kind == SCH else {}
    out, flags, _ = _run(emu, kind, spots, None, [Cm.T / N_STEPS] * N_INST, **kw)
    bad = np.zeros(flags.shape, dtype=bool)
    bad[1, 3] = bad[2, 9] = bad[4, 0] = True
    assert ((flags == R.OFF_GRID) == bad).all() and (flags[~bad] == 0).all()
    assert np.isnan(out[:, :, :][np.broadcast_to(bad[:, None, :], out.shape)]).all()
    ok, _, _ = _run(emu, kind, spots_n, None, [Cm.T / N_STEPS] * N_INST, **kw)
    keep = np.broadcast_to(~bad[:, None, :], out.shape)
    assert np.array_equal(out[keep], ok[keep])  # the other samples are untouched
