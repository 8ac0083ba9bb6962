"""CPU-only check of the Bates sub-step under the wave emulator (tests/emu/emu_jumps.cpp): hadi_jump_matrix_kernel against the
numpy generator of tests/jumps_ref.py, entry by entry, and hadi_jump_kernel behind the emulated streaming ring and strips on
every streaming layout (1, 2, 4, 8 nodes per lane, two wavefronts per row), fields against tests/jumps_ref.py at this file
family's bound, 1e-10 of the instance's max|U_ref|, on well-conditioned grids (asserted).  The product's setup and pack kernels
build the inputs; the weights and the matrices are built as the library's host code builds them.  Invariants: no pad slot of the
packed state changes against the same run without jumps; a finished or zero-intensity instance is its plain run bit for bit; an
instance's result does not depend on the batch around it, on a shared matrix or on how many instances ride on one block.
tests/test_jumps_ref.py shows that each class of mistake in the generator moves the reference price by more than 1e-2."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import common as Cm
import jumps_ref as JR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_jumps.so")
_dp = C.POINTER(C.c_double)

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH = {0: Cm.THETA, 1: 0.5, 2: 1.0 / 3.0, 3: 0.5 + math.sqrt(3.0) / 6.0}
# per-instance jump laws, cycled through the batch: the three sets of the accuracy table, a fourth, and one with intensity 0
LAM, MU, SIG = (0.5, 2.0, 0.3, 1.0, 0.0), (-0.10, -0.05, 0.10, -0.20, 0.05), (0.15, 0.10, 0.30, 0.25, 0.20)


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_jumps.cpp", "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp,
                               os.path.join(HERE, "emu", "emu_jumps.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_jumps_packed_size.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


_GRIDS = {}


def grids(m1, m2, n, same=False):
    """Well-conditioned batch (asserted), built once per shape and left unchanged.  same: every instance on instance 0's grid."""
    if (m1, m2, n, same) not in _GRIDS:
        strikes = Cm.well_conditioned_strikes(m1, 1) * n if same else Cm.well_conditioned_strikes(m1, n)
        g = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
        Cm.assert_well_conditioned(g[2], g[3])
        _GRIDS[(m1, m2, n, same)] = (strikes,) + g
    return _GRIDS[(m1, m2, n, same)]


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


def run(emu, m1, m2, n, N_i, dt_i, law, scheme=0, put=False, div=False, strip=None, shared=False, ipg=1, same=False):
    """(field [n][m], packed state, pad mask, the word of the shared-grid check).  law: (lam, mu, sig) [n] each, or None = no jump
    tables at all."""
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n, same)
    par8 = np.array([list(MODEL) + [dt_i[k], N_i[k], strikes[k] if put else 0.0, 1.0 if put else 0.0] for k in range(n)])
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    Uout = np.zeros_like(Uin)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in Cm.DIVS] if div else [None] * 3
    lam, mu, sig = (None, None, None) if law is None else (np.ascontiguousarray(x, dtype=np.float64) for x in law)
    size = emu.emu_jumps_packed_size(n, m1, m2)
    P, pad, stat = np.zeros(size), np.zeros(size, dtype=np.uint8), C.c_int(-1)
    if strip is not None:
        emu.emu_set_tuning(b"strip", strip)
    try:
        rc = emu.emu_jumps(n, m1, m2, C.c_double(TH[scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(vs), _P(vv),
                           _P(ds), _P(dv), _P(Uin), scheme, len(dd[0]) if div else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]),
                           _P(lam), _P(mu), _P(sig), int(shared), ipg, _P(Uout), _P(P), pad.ctypes.data_as(C.c_void_p), C.byref(stat))
    finally:
        emu.emu_set_tuning(b"reset", 0)
    assert rc == 0, rc
    assert emu.emu_take_error() == 0
    return Uout, P, pad.astype(bool), stat.value


def reference(m1, m2, n, N_i, dt_i, law, scheme=0, put=False, div=False, same=False):
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n, same)
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    return JR.solve_batch(m1, m2, max(N_i), dt_i[0], TH[scheme], Cm.R_D, Cm.R_F, *MODEL, vs, vv, ds, dv, Uin, *law,
                          dividends=Cm.DIVS if div else None, put_strikes=strikes if put else None, scheme=scheme, N_i=N_i, dt_i=dt_i)


def check(emu, name, m1, m2, n, N_i, dt_i, law, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ("scheme", "put", "div", "same")}
    U, P, pad, _ = run(emu, m1, m2, n, N_i, dt_i, law, **kw)
    Uo = reference(m1, m2, n, N_i, dt_i, law, **ref_kw)
    err = np.abs(U - Uo).max(axis=1) / np.abs(Uo).max(axis=1)
    print("%s %dx%d: %.2e of max|U_ref|" % (name, m1, m2, err.max()))
    assert np.isfinite(U).all() and err.max() <= 1e-10, (name, err)
    # the pad slots of the state: exactly what the same run leaves there without jumps; the nodes did move
    plain_kw = {k: v for k, v in kw.items() if k not in ("shared", "ipg")}
    U0, P0, pad0, _ = run(emu, m1, m2, n, N_i, dt_i, None, **plain_kw)
    assert pad.any() and np.array_equal(pad, pad0) and np.array_equal(P[pad], P0[pad]), name
    moved = [k for k in range(n) if law[0][k] != 0.0]
    assert moved and all(np.abs(U[k] - U0[k]).max() > 1e-6 * np.abs(Uo[k]).max() for k in moved), name
    # a zero-intensity instance is its plain run, bit for bit
    assert all(np.array_equal(U[k], U0[k]) for k in range(n) if law[0][k] == 0.0), name
    return U, U0


def uniform(n, N):
    return [N] * n, [Cm.T / N] * n


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", [50, 100, 200, 300, 600])
def test_matrix_kernel_against_the_numpy_generator(emu, m1):
    """Elementwise within 1e-13 max(1, |kbar| s_i / min(ds_{i-1}, ds_i)): a few ulp of erfc on entries of that magnitude, with three
    orders of margin."""
    vs = grids(m1, 8, 1)[1][0]
    ds = np.diff(vs)
    for lam, mu, sig in ([(LAM[0], MU[0], SIG[0])] if m1 > 200 else list(zip(LAM, MU, SIG))[:3]):
        G = np.full((m1 + 1, m1 + 1), np.nan)
        assert emu.emu_jump_matrix(m1, _P(vs), C.c_double(mu), C.c_double(sig), _P(G)) == 0
        Gr = JR.generator(vs, mu, sig)
        hmin = np.minimum(np.r_[ds[0], ds], np.r_[ds, ds[-1]])
        bound = 1e-13 * np.maximum(1.0, abs(JR.kbar(mu, sig)) * vs / hmin)
        worst = (np.abs(G - Gr) / bound[:, None]).max()
        print("m1 = %d (%g, %g): worst entry at %.3f of its bound, |G 1| = %.2e" % (m1, mu, sig, worst, np.abs(G @ np.ones(m1 + 1)).max()))
        assert np.isfinite(G).all() and worst <= 1.0
        assert not G[0].any()


# ---- the sweep on every streaming layout ---------------------------------------------------------------------------------------------
# 1, 2, 4, 8 nodes per lane and two wavefronts per row; N <= 10
SHAPES = [(50, 25, 8), (100, 12, 6), (200, 12, 4), (300, 12, 3), (600, 8, 2)]
VARIANTS = [(False, False), (True, True)]


@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("put,div", VARIANTS, ids=["EU-call", "DIV-put"])
def test_every_layout(emu, m1, m2, N, put, div):
    """Two instances with their own jump laws (three on the small grids) behind the plan's own streaming kernels."""
    n = 3 if m1 <= 100 else 2
    check(emu, "layout", m1, m2, n, *uniform(n, N), laws(n, first=1 if put else 0), put=put, div=div)


@pytest.mark.parametrize("put,div", [(True, False), (False, True)], ids=["EU-put", "DIV-call"])
@pytest.mark.parametrize("m1,m2,N,strip", [(50, 25, 6, 0), (100, 12, 5, 0), (100, 12, 5, 1)], ids=["50x25-ring", "100x12-ring", "100x12-strips"])
def test_ring_and_strips(emu, m1, m2, N, strip, put, div):
    check(emu, "pinned", m1, m2, 3, *uniform(3, N), laws(3, first=2), put=put, div=div, strip=strip)


@pytest.mark.parametrize("scheme", [2, 3], ids=["MCS", "HV"])
@pytest.mark.parametrize("m1,m2,N,strip", [(50, 25, 5, 0), (100, 12, 4, 1)], ids=["50x25-ring", "100x12-strips"])
def test_predictor_corrector_schemes(emu, scheme, m1, m2, N, strip):
    """The sub-step follows the corrector's column pass."""
    check(emu, "scheme %d" % scheme, m1, m2, 3, *uniform(3, N), laws(3), scheme=scheme, strip=strip)


N_MIX = [5, 8, 3, 7, 6]
DT_MIX = [0.5 / 5, Cm.T / 8, 0.25 / 3, 0.8 / 7, 0.6 / 6]


@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 12)])
def test_mixed_step_grids_and_jump_laws(emu, m1, m2, div):
    """Every instance its own (N, dt, lambda, mu_J, sigma_J) and dividend dating: instances finish at steps 3, 5, 6, 7 and 8 and are
    left alone afterwards; the last one has intensity 0."""
    check(emu, "mixed", m1, m2, 5, N_MIX, DT_MIX, laws(5), put=True, div=div)


def test_one_instance_equals_the_same_instance_in_a_batch_of_five(emu):
    """Bit for bit, with mixed step grids around it: an instance's result depends neither on its place in the batch nor on what
    else is in it."""
    m1, m2 = 50, 25
    assert grids(m1, m2, 1)[0][0] == grids(m1, m2, 5)[0][0]
    law = laws(5)
    U5, _, _, _ = run(emu, m1, m2, 5, N_MIX, DT_MIX, law, put=True)
    U1, _, _, _ = run(emu, m1, m2, 1, N_MIX[:1], DT_MIX[:1], tuple(x[:1] for x in law), put=True)
    assert np.array_equal(U1[0], U5[0])
    # ... and the finished ones: instance 2 (3 steps) inside the batch of five (8 steps) against the first three alone
    U3, _, _, _ = run(emu, m1, m2, 3, N_MIX[:3], DT_MIX[:3], tuple(x[:3] for x in law), put=True)
    assert np.array_equal(U3, U5[:3])


# ---- one matrix for the batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,ipg", [(50, 25, 1), (50, 25, 2), (100, 12, 4), (200, 12, 2)])
def test_shared_matrix(emu, m1, m2, ipg):
    """Every instance on instance 0's grid with one (mu_J, sigma_J); own intensities (one of them 0) and step grids.  Several
    instances ride on one staged strip (ipg); the result is that of the per-instance matrices, bit for bit, and the reference's."""
    n = 3 if m1 > 100 else 5
    N_i, dt_i = N_MIX[:n], DT_MIX[:n]
    law = (np.array([LAM[(k + 3) % 5] for k in range(n)]), np.full(n, MU[0]), np.full(n, SIG[0]))
    U, _ = check(emu, "shared ipg %d" % ipg, m1, m2, n, N_i, dt_i, law, same=True, shared=True, ipg=ipg)
    Up, _, _, stat = run(emu, m1, m2, n, N_i, dt_i, law, same=True)
    assert np.array_equal(U, Up) and stat == 0


def test_shared_grid_promise_is_checked(emu):
    law = (np.full(3, 0.5), np.full(3, MU[0]), np.full(3, SIG[0]))
    assert run(emu, 50, 25, 3, *uniform(3, 2), law, same=True, shared=True)[3] == 0
    assert run(emu, 50, 25, 3, *uniform(3, 2), law, same=False, shared=True)[3] == 1


def test_no_jump_tables_is_the_plain_run_bit_for_bit(emu):
    """emu_solve (emu_driver.cpp) on the same inputs; and all-zero intensities take the same path."""
    m1, m2, n, N = 100, 12, 3, 4
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n)
    U = U0.copy()
    par = np.array([list(MODEL)] * n)
    rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(TH[0]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par), 0, _P(vs),
                       _P(vv), _P(ds), _P(dv), _P(U), None, None, 8 * 256, 0, None, None, None, 64, 0, 0, None, None, None)
    assert rc == 0, rc
    assert np.array_equal(run(emu, m1, m2, n, *uniform(n, N), None)[0], U)
    zero = (np.zeros(n), np.full(n, -0.1), np.full(n, 0.15))
    assert np.array_equal(run(emu, m1, m2, n, *uniform(n, N), zero)[0], U)


# ---- the route of a jump call -------------------------------------------------------------------------------------------------------------
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING = range(6)  # enum HadiRouteKind
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"


def route(emu, n, m1, m2, jumps, variant=0, scheme=0, tuning="", cus=256, theta=Cm.THETA, team=0):
    arr = (C.c_int * 16)(cus, n, m1, m2, variant, scheme, 0, 0, 0, 0, 0, int(variant == 2), 1, 0, 0, team)
    o, subs, desc = (C.c_longlong * 16)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
    emu.emu_route_jumps.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    assert emu.emu_route_jumps(arr, theta, tuning.encode(), int(jumps), o, subs, 64, desc, 1024) == 0
    return list(o), [tuple(subs[4 * k:4 * k + 4]) for k in range(o[3])], desc.value.decode()


def test_route_is_always_streaming(emu):
    """No whole-loop LDS kernel, no resident sweep, no team launch; U_temp is grown; the loop stays graphable."""
    cases = [(3, 50, 25, 0, "", SMALL), (300, 50, 25, 0, "", SMALL_SEQ), (600, 50, 25, 0, "", SMALL_SEQ2),
             (3, 50, 25, 0, "small_seq=1,small_pairs=1", SMALL_SEQ2), (300, 50, 25, 2, "", SMALL_SCH), (3, 50, 25, 2, "small_sch=1", SMALL_SCH),
             (20, 300, 80, 0, "", STREAMING), (4, 300, 140, 0, "", TEAM)]
    for n, m1, m2, scheme, tuning, kind in cases:
        o0, _, d0 = route(emu, n, m1, m2, False, scheme=scheme, tuning=tuning, theta=TH[scheme])
        o1, _, d1 = route(emu, n, m1, m2, True, scheme=scheme, tuning=tuning, theta=TH[scheme])
        assert o0[1] == kind and o0[15] == 0 and "Bates" not in d0, (n, m1, m2, o0)
        assert o1[1] == STREAMING and o1[15] == 1 and o1[10] == 1 and o1[14] == o0[14] and d1.endswith(JUMP_WORDS) and "row pass" in d1, d1
    for n, m1, m2, tuning in ((256, 300, 80, "resident_sweep=1"), (256, 512, 256, "")):
        o, subs, d = route(emu, n, m1, m2, False, tuning=tuning)
        assert o[6] == 1 and "hadi_sweep_resident" in d, d
        o, subs, d = route(emu, n, m1, m2, True, tuning=tuning)
        assert o[1] == STREAMING and o[6] == 0 and not any(s[3] for s in subs) and "hadi_sweep_resident" not in d and d.endswith(JUMP_WORDS), d
    o, subs, d = route(emu, 320, 512, 256, True)  # a round and a remainder, side by side on two streams
    assert [s[1] for s in subs] == [256, 64] and o[4] == 1 and "two streams" in d, d


def test_recorded_routes(emu):
    """tests/golden/route_selection_jumps.json, recorded on the MI355X (tools/record_jumps_routes.py): hadi_route and
    hadi_describe_route reproduce the description of every recorded jump call and of the plain call of the same batch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_jumps_routes as R
    fix = json.load(open(R.FIXTURE))
    assert len(fix["cases"]) == len(R.CASES) >= 10
    for row in fix["cases"]:
        tuning = ",".join("%s=%d" % kv for kv in sorted(row["tuning"].items()))
        kw = dict(scheme=row["scheme"], tuning=tuning, cus=fix["cu_count"], theta=R.TH[row["scheme"]])
        o0, _, _ = route(emu, row["n"], row["m1"], row["m2"], False, **kw)
        team = 1 if o0[1] == TEAM else 0  # (a team launch is taken to have run)
        assert route(emu, row["n"], row["m1"], row["m2"], False, team=team, **kw)[2] == row["plain"], row["name"]
        o1, _, d1 = route(emu, row["n"], row["m1"], row["m2"], True, **kw)
        assert d1 == row["bates"] and o1[15] == 1 and o1[1] == STREAMING and d1.endswith(JUMP_WORDS), (row["name"], d1)
