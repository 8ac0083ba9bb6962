"""CPU-only check of the nine-group batch of hadi_compute_jacobian_bates_jumps under the wave emulator (tests/emu/emu_jumps8.cpp):
hadi_jump_sel_kernel behind the streaming kernels -- three matrix sets picked by group, the groups 0 .. 6 of a source instance on
one staged strip -- against tests/jumps8_ref.py (bound: 1e-10 of the instance's max|U_ref| on well-conditioned grids, as
tests/test_emu_jumps.py), against the six-group batch through hadi_jump_kernel bit for bit, and over every way of putting the
instances onto strips and into sub-batches, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common as Cm
import jumps8_ref as J8
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_jumps8.so")
_dp = C.POINTER(C.c_double)
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
EPS = 1e-6
G = 9
LAM, MU, SIG = (0.5, 0.0, 2.0), (-0.10, 0.05, -0.05), (0.15, 0.20, 0.10)  # instance 1: intensity 0


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_jumps8.cpp", "emu_jumps.cpp", "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp,
                               os.path.join(HERE, "emu", "emu_jumps8.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_jumps_packed_size.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


class Batch:
    """The nine groups of n0 calls as jacobian_common lays them out: the caller's rows repeated, one parameter bumped per group,
    group 5's v-grid rebuilt for V_0 + eps."""

    def __init__(self, m1, m2, n0, N_i, same=False):
        self.m1, self.m2, self.n0, self.N_i = m1, m2, n0, list(N_i)
        self.V_0 = Cm.v0_for(m2)
        self.strikes = Cm.well_conditioned_strikes(m1, 1) * n0 if same else Cm.well_conditioned_strikes(m1, n0)
        self.vs, vv, self.ds, dv, self.U0 = Cm.oracle_grids(m1, m2, self.strikes, V0=self.V_0)
        Cm.assert_well_conditioned(self.ds, dv)
        self.dt_i = [Cm.T / N for N in self.N_i]
        rows, vvs, dvs = [], [], []
        for g in range(G):
            rho, sigma, kappa, eta = (MODEL[q] + (EPS if g == (4, 3, 1, 2)[q] else 0.0) for q in range(4))
            gv, gdv = O.rebuild_variance(m2, self.V_0 + (EPS if g == 5 else 0.0))
            for k in range(n0):
                rows.append([rho, sigma, kappa, eta, self.dt_i[k], self.N_i[k], 0.0, 0.0])
                vvs.append(gv)
                dvs.append(gdv)
        self.par8 = np.array(rows)
        self.vs9, self.ds9 = np.ascontiguousarray(np.tile(self.vs, (G, 1))), np.ascontiguousarray(np.tile(self.ds, (G, 1)))
        self.vv9, self.dv9 = np.ascontiguousarray(np.stack(vvs)), np.ascontiguousarray(np.stack(dvs))
        Cm.assert_well_conditioned(self.ds9, self.dv9)

    def law(self, shared=False):
        lam = np.array([LAM[k % 3] for k in range(self.n0)])
        if shared:
            return lam, np.full(self.n0, MU[0]), np.full(self.n0, SIG[0])
        return lam, np.array([MU[k % 3] for k in range(self.n0)]), np.array([SIG[k % 3] for k in range(self.n0)])

    def run(self, emu, law, shared=0, share=1, cap=7, split=0, pads=False):
        n = G * self.n0
        m = (self.m1 + 1) * (self.m2 + 1)
        out = np.zeros((n, m))
        size = emu.emu_jumps_packed_size(n, self.m1, self.m2)
        P, pad = np.zeros(size), np.zeros(size, dtype=np.uint8)
        lam, mu, sig = (np.ascontiguousarray(x, dtype=np.float64) for x in law)
        rc = emu.emu_jumps8(self.n0, self.m1, self.m2, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(self.par8),
                            _P(self.vs9), _P(self.vv9), _P(self.ds9), _P(self.dv9), _P(self.U0), 0, _P(lam), _P(mu), _P(sig),
                            C.c_double(EPS), shared, share, cap, split, _P(out), _P(P), pad.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        assert emu.emu_take_error() == 0
        return (out, P, pad.astype(bool)) if pads else out

    def six_groups_old_kernel(self, emu, law):
        """The groups 0 .. 5 as the six-group batch of hadi_compute_jacobian_bates runs them: hadi_jump_kernel, one matrix per
        instance of the batch."""
        n = 6 * self.n0
        m = (self.m1 + 1) * (self.m2 + 1)
        out = np.zeros((n, m))
        rep = [np.ascontiguousarray(np.tile(x, 6)) for x in law]
        U6 = np.ascontiguousarray(np.tile(self.U0, (6, 1)))
        rc = emu.emu_jumps(n, self.m1, self.m2, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(self.par8[:n].copy()),
                           _P(self.vs9[:n].copy()), _P(self.vv9[:n].copy()), _P(self.ds9[:n].copy()), _P(self.dv9[:n].copy()), _P(U6), 0,
                           0, None, None, None, _P(rep[0]), _P(rep[1]), _P(rep[2]), 0, 1, _P(out), None, None, None)
        assert rc == 0, rc
        assert emu.emu_take_error() == 0
        return out

    def reference(self, law):
        """[9 n0][m] fields of tests/jumps8_ref.py."""
        kw = dict(N_i=self.N_i, dt_i=self.dt_i)
        _, fields = J8.group_prices(self.m1, self.m2, max(self.N_i), self.dt_i[0], Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, Cm.S_0, self.V_0,
                                    self.vs, self.ds, self.U0, *law, eps=EPS, **kw)
        return np.concatenate(fields)


SHAPES = [(50, 25, 3, (3, 2, 3)), (600, 8, 2, (2, 2))]
_CACHE = {}


def case(emu, m1, m2, n0, N_i):
    """The batch, its default run and its reference, computed once per shape and left unchanged."""
    key = (m1, m2, n0, N_i)
    if key not in _CACHE:
        b = Batch(m1, m2, n0, N_i)
        U, P, pad = b.run(emu, b.law(), pads=True)
        Uo = b.reference(b.law())
        for a in (U, P, Uo):
            a.setflags(write=False)
        _CACHE[key] = (b, U, P, pad, Uo)
    return _CACHE[key]


@pytest.mark.parametrize("m1,m2,n0,N_i", SHAPES, ids=["50x25x3", "600x8x2"])
def test_fields_of_all_nine_groups(emu, m1, m2, n0, N_i):
    b, U, P, pad, Uo = case(emu, m1, m2, n0, N_i)
    err = np.abs(U - Uo).max(axis=1) / np.abs(Uo).max(axis=1)
    print("%dx%d x %d: %.2e of max|U_ref| over the nine groups" % (m1, m2, n0, err.max()))
    assert np.isfinite(U).all() and err.max() <= 1e-10, err
    # every bumped group moved its field (the bump is seen), the matrix sets 1 and 2 included
    lam = b.law()[0]
    for g in range(1, G):
        for k in range(n0):
            same = np.array_equal(U[g * n0 + k], U[k])
            assert same == (g in (7, 8) and lam[k] == 0.0), (g, k)


@pytest.mark.parametrize("m1,m2,n0,N_i", SHAPES, ids=["50x25x3", "600x8x2"])
def test_groups_0_to_5_are_the_six_group_batch_bit_for_bit(emu, m1, m2, n0, N_i):
    b, U, *_ = case(emu, m1, m2, n0, N_i)
    assert np.array_equal(U[:6 * n0], b.six_groups_old_kernel(emu, b.law()))


LISTS = [dict(share=0, cap=1), dict(share=1, cap=1), dict(share=1, cap=3), dict(share=0, cap=4), dict(share=1, cap=7, split=5),
         dict(share=1, cap=2, split=20), dict(share=0, cap=1, split=13)]


@pytest.mark.parametrize("kw", LISTS, ids=["-".join("%s%d" % i for i in kw.items()) for kw in LISTS])
def test_bits_do_not_depend_on_the_lists(emu, kw):
    """One instance per block, strips shared by 1, 2, 3 or 7 instances, runs of four consecutive instances that change matrices, and
    two sub-batches cut inside a group: every element of the packed state, pad slots included, is the same."""
    b, U, P, pad, _ = case(emu, *SHAPES[0])
    V, Q, pad2 = b.run(emu, b.law(), pads=True, **kw)
    assert np.array_equal(U, V) and np.array_equal(P, Q) and np.array_equal(pad, pad2)


def test_two_wavefront_rows_with_and_without_sharing(emu):
    b, U, P, *_ = case(emu, *SHAPES[1])
    V, Q, _ = b.run(emu, b.law(), share=0, cap=1, split=7, pads=True)
    assert np.array_equal(U, V) and np.array_equal(P, Q)


def test_shared_matrices(emu):
    """One grid and one (mu_J, sigma_J): three matrices for the batch, runs of consecutive instances on one strip -- the result of
    the per-instance matrices, bit for bit."""
    b = Batch(50, 25, 3, (3, 3, 3), same=True)
    law = b.law(shared=True)
    U = b.run(emu, law)
    for cap in (1, 4, 8):
        assert np.array_equal(U, b.run(emu, law, shared=1, share=0, cap=cap))
    assert not np.array_equal(U[0], U[2])  # (same grid and matrix, another intensity)


def test_finished_and_zero_weight_instances_are_untouched(emu):
    m1, m2, n0, N_i = SHAPES[0]
    b, U, P, pad, _ = case(emu, m1, m2, n0, N_i)
    # instance 1 has N = 2 in a batch that runs 3 steps: in every group its field is that of the batch that stops after 2
    short = Batch(m1, m2, n0, (2, 2, 2))
    V = short.run(emu, short.law())
    for g in range(G):
        assert np.array_equal(U[g * n0 + 1], V[g * n0 + 1]), g
    # instance 1 has intensity 0: outside group 6 its field is the plain sweep's (no jump tables at all), bit for bit
    n = 6 * n0
    plain = np.zeros((n, (m1 + 1) * (m2 + 1)))
    U6 = np.ascontiguousarray(np.tile(b.U0, (6, 1)))
    rc = emu.emu_jumps(n, m1, m2, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(b.par8[:n].copy()), _P(b.vs9[:n].copy()),
                       _P(b.vv9[:n].copy()), _P(b.ds9[:n].copy()), _P(b.dv9[:n].copy()), _P(U6), 0, 0, None, None, None, None, None, None,
                       0, 1, _P(plain), None, None, None)
    assert rc == 0 and emu.emu_take_error() == 0
    for g in range(6):
        assert np.array_equal(U[g * n0 + 1], plain[g * n0 + 1]), g
    assert np.array_equal(U[7 * n0 + 1], U[1]) and np.array_equal(U[8 * n0 + 1], U[1])
    assert not np.array_equal(U[6 * n0 + 1], U[1])  # (group 6 jumps with eps delta_t)
    # the pad slots: what the plain nine-group run leaves there
    zero = (np.zeros(n0), b.law()[1], b.law()[2])
    _, P0, pad0 = b.run(emu, zero, pads=True)
    assert pad.any() and np.array_equal(pad, pad0) and np.array_equal(P[pad], P0[pad])


def test_every_instance_is_on_exactly_one_list(emu):
    """hadi_jump_sel_list over sub-batches of every offset and length of a 9 x 5 batch: each instance once, no list beyond the
    launch, a shared strip never mixes matrices, and no list longer than the cap."""
    n_src = 5
    n = G * n_src
    longest = C.c_int(0)
    seen7 = False
    for share, per in ((1, n_src), (0, n_src), (0, 1)):
        for cap in (1, 2, 3, 7):
            for inst0 in range(0, n, 3):
                for cnt in (1, 2, n_src - 1, n_src, n_src + 1, 2 * n_src + 3, n - inst0):
                    if cnt < 1 or inst0 + cnt > n:
                        continue
                    cover = (C.c_int * cnt)()
                    ngrp = emu.emu_jump_sel_lists(inst0, n_src, per, share, cap, cnt, cover, C.byref(longest))
                    assert ngrp > 0 and list(cover) == [1] * cnt, (share, per, cap, inst0, cnt, list(cover))
                    assert longest.value <= cap
                    seen7 = seen7 or (share and longest.value == 7)
    assert seen7  # (the seven set-0 groups of a source instance do ride on one strip)
