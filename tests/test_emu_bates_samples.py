"""CPU-only check of a sampled Bates ladder under the wave emulator (tests/emu/emu_bates_samples.cpp): hadi_small_jump_kernel -- the
block kernel of the small path with the jump sub-step between the column pass and the snapshot -- and the streaming combination
(copy, hadi_jump_kernel / hadi_jump_sel_kernel, then hadi_sample_kernel), against tests/bates_samples_ref.py.

Bound, the sample calls' (tests/test_emu_samples.py): every sample within 1e-10 sum|w| |scale| max|U_ref| on well-conditioned grids
(asserted).  Shapes of the whole-loop kernel: 50x25 (B = 1, two row blocks of 16 and 10 rows, the last slot block holds the i = 0 slot
and pads), 100x12 (B = 2, 13 rows: one row block), 50x32 (33 rows: a last row block of one row), W = 4 and 8; and every row of
tests/bates_domain_cases.py (the whole-loop shapes of event_cases.LDS_ROWS and 128 x the largest m2 the route function admits, found
with it and never written down) at both widths with N = 3.  Invariants: an
instance with a_k = 0 is its plain run bit for bit; no pad slot of the packed state differs from the same run without jumps; a
shared matrix gives the per-instance matrices' bits; the nine groups pick their three matrix sets.  (A ladder shares the step
indices -- N_i is refused --, so no instance finishes before another inside such a call.)  The route function: jumps without
samples still stream; jumps with samples follow "jump_small"; refused shapes stream."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import bates_domain_cases as BD
import bates_samples_ref as BS
import common as Cm
import samples_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_bates_samples.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
LAM, MU, SIG = (0.5, 2.0, 0.0, 1.0, 0.3), (-0.10, -0.05, 0.05, -0.20, 0.10), (0.15, 0.10, 0.20, 0.25, 0.30)  # the third: intensity 0
SNAPS = [2, 5, 6]


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_bates_samples.cpp", "emu_jumps.cpp", "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp,
                               os.path.join(HERE, "emu", "emu_bates_samples.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_jumps_packed_size.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


_GRIDS = {}


def grids(m1, m2, n, same=False):
    """Well-conditioned batch (asserted) with its ten spots per instance, built once per shape and left unchanged."""
    if (m1, m2, n, same) not in _GRIDS:
        strikes = Cm.well_conditioned_strikes(m1, 1) * n if same else Cm.well_conditioned_strikes(m1, n)
        g = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
        Cm.assert_well_conditioned(g[2], g[3])
        spots = np.ascontiguousarray(np.stack([SR.kernel_test_spots(g[0][k], Cm.S_0) for k in range(n)]))
        _GRIDS[(m1, m2, n, same)] = (strikes,) + g + (spots,)
    return _GRIDS[(m1, m2, n, same)]


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


def launch(emu, how, m1, m2, n0, par8, vs, vv, ds, dv, U, lam, musig, sets, shared, V_0, v0_i, spots, scales, snaps, div=False):
    """The raw entry point on a batch of par8.shape[0] instances.  Returns (samples, packed state, pad mask, shared-grid word)."""
    n = par8.shape[0]
    n_samp = spots.shape[1]
    out = np.full((n, len(snaps), n_samp), np.nan)
    flags = np.full((n, n_samp), -1, dtype=np.int32)
    size = emu.emu_jumps_packed_size(n, m1, m2)
    P, pad, stat = np.zeros(size), np.zeros(size, dtype=np.uint8), C.c_int(-1)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in Cm.DIVS] if div else [None] * 3
    sn = np.ascontiguousarray(snaps, dtype=np.int32)
    ms = None if musig is None else np.ascontiguousarray(musig, dtype=np.float64)
    lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
    sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
    v0i = None if v0_i is None else np.ascontiguousarray(v0_i, dtype=np.float64)
    rc = emu.emu_bates_samples(n, n0, m1, m2, C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(vs), _P(vv), _P(ds),
                               _P(dv), _P(U), len(dd[0]) if div else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]), _P(lam), _P(ms),
                               0 if ms is None else ms.size // 2, sets, int(shared), how, C.c_double(V_0), _P(v0i), n_samp, _P(spots), _P(sc),
                               spots.shape[0], len(snaps), sn.ctypes.data_as(_ip), _P(out), flags.ctypes.data_as(_ip), _P(P),
                               pad.ctypes.data_as(C.c_void_p), C.byref(stat))
    assert rc == 0, rc
    assert emu.emu_take_error() == 0 and (flags == 0).all()
    return out, P, pad.astype(bool), stat.value


def run(emu, how, m1, m2, n, N, law, put=False, div=False, dts=None, shared=False, same=False, snaps=SNAPS):
    """A plain batch of n instances; law (lam, mu, sig) [n] each, or None: no jump tables at all."""
    strikes, vs, vv, ds, dv, U0, spots = grids(m1, m2, n, same)
    dt = dts or [Cm.T / N] * n
    par8 = np.array([list(MODEL) + [dt[k], N, strikes[k] if put else 0.0, 1.0 if put else 0.0] for k in range(n)])
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    lam = musig = None
    if law is not None:
        lam = law[0]
        musig = [[law[1][0], law[2][0]]] if shared else [[law[1][k], law[2][k]] for k in range(n)]
    return launch(emu, how, m1, m2, n, par8, vs, vv, ds, dv, Uin, lam, musig, 1, shared, Cm.v0_for(m2), None, spots, None, snaps, div)


def reference(m1, m2, n, N, law, put=False, div=False, dts=None, same=False, snaps=SNAPS):
    strikes, vs, vv, ds, dv, U0, spots = grids(m1, m2, n, same)
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    return BS.sample_ladder(m1, m2, snaps, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, vs, vv, ds, dv, Uin, Cm.v0_for(m2), spots, None, *law,
                            dividends=Cm.DIVS if div else None, put_strikes=strikes if put else None, dt_i=dts)


def within_bound(name, out, ref):
    vals, amp, top = ref
    bound = 1e-10 * amp * top[:, :, None]
    worst = (np.abs(out - vals) / bound).max()
    print("%s: worst |diff| / bound %.2e" % (name, worst))
    assert np.isfinite(out).all() and worst <= 1.0, (name, worst)


def check(emu, name, how, m1, m2, n, N, law, snaps=SNAPS, **kw):
    out, P, pad, _ = run(emu, how, m1, m2, n, N, law, snaps=snaps, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("put", "div", "dts", "same")}
    within_bound(name, out, reference(m1, m2, n, N, law, snaps=snaps, **ref_kw))
    # the same run without jump tables: the pad slots of the state are what it leaves there, the nodes did move
    out0, P0, pad0, _ = run(emu, how, m1, m2, n, N, None, snaps=snaps, **{k: v for k, v in kw.items() if k != "shared"})
    assert pad.any() and np.array_equal(pad, pad0) and np.array_equal(P[pad], P0[pad]), name
    for k in range(n):
        if law[0][k] == 0.0:  # bit for bit its plain run
            assert np.array_equal(out[k], out0[k]), (name, k)
        else:
            assert np.abs(out[k] - out0[k]).max() > 1e-6, (name, k)
    return out


WHOLE = [("50x25-W8-call", 8, 50, 25, 6, SNAPS, dict()),
         ("50x25-W4-DIV-put", 4, 50, 25, 6, SNAPS, dict(put=True, div=True)),
         ("100x12-W4-DIV-call", 4, 100, 12, 4, [1, 3, 4], dict(div=True)),
         ("100x12-W8-put", 8, 100, 12, 4, [2, 4], dict(put=True)),
         ("50x32-W8-call", 8, 50, 32, 3, [1, 3], dict())]
# ... and every row of bates_domain_cases' table at both widths (m2 None: the largest m2 the route admits at 128, found below)
WHOLE += [("%dx%d-W%d" % (r.m1, r.m2, W), W, r.m1, r.m2, 3, [1, 3], dict()) for r in BD.FIXED for W in BD.WIDTHS
          if ("%dx%d-W%d-call" % (r.m1, r.m2, W)) not in [w[0] for w in WHOLE]]
WHOLE += [("%dxlargest-W%d" % (BD.LARGEST_M1, W), W, BD.LARGEST_M1, None, 3, [1, 3], dict()) for W in BD.WIDTHS]


def takes_the_loop(emu, m1, m2, must=None):
    """The emulator's route function with "jump_small" = 1: does a sampled Bates ladder take hadi_small_jump_kernel<2,..> there?"""
    o, d = route(emu, 3, m1, m2, True, n_snap=2, n_samp=10, tuning="jump_small=1")
    loop = d.startswith("hadi_small_jump_kernel<2,")
    assert loop == (o[1] == SMALL_JUMP) and (loop or (o[1] == STREAMING and d.endswith(JUMP_WORDS) and "row pass" in d)), d
    return loop


def largest_m2(emu):
    m2 = BD.largest_m2(lambda m1, m2: takes_the_loop(emu, m1, m2))
    assert not takes_the_loop(emu, BD.LARGEST_M1, m2 + 1)  # (streams: the words are asserted in takes_the_loop)
    return m2


@pytest.mark.parametrize("name,how,m1,m2,N,snaps,kw", WHOLE, ids=[w[0] for w in WHOLE])
def test_whole_loop_kernel(emu, name, how, m1, m2, N, snaps, kw):
    if m2 is None:
        m2 = largest_m2(emu)
        row = BD.shapes(m2)[-1]
        name = "%dx%d-W%d" % (m1, m2, how)
    else:
        row = next((r for r in BD.FIXED if (r.m1, r.m2) == (m1, m2)), None)
    if row is not None:
        print(BD.what(row))
    o4 = (C.c_longlong * 4)()
    assert emu.emu_bates_samples_layout(m1, m2, 3, o4) == 0 and 0 < o4[3] <= 76 * 1024
    assert (o4[0], o4[1], o4[2]) == (BD.geometry(m1, m2)[0], BD.geometry(m1, m2)[1], m2 + 1)
    check(emu, name, how, m1, m2, 3, N, laws(3), snaps=snaps, **kw)


def test_whole_loop_kernel_with_delta_t_i(emu):
    dts = [Cm.T / 6, 0.5 / 6, 0.8 / 6]
    check(emu, "delta_t_i", 8, 50, 25, 3, 6, laws(3, first=3), dts=dts, div=True)


@pytest.mark.parametrize("how,m1,m2,N", [(0, 50, 25, 6), (0, 100, 12, 4)], ids=["50x25", "100x12"])
def test_streaming_combination(emu, how, m1, m2, N):
    """The jump kernel, then the sample kernel, behind the plan's own pass kernels."""
    check(emu, "streaming", how, m1, m2, 3, N, laws(3), snaps=[2, N], put=(m1 == 100), div=True)


@pytest.mark.parametrize("how", [8, 0], ids=["whole-loop", "streaming"])
def test_shared_matrix_gives_the_per_instance_bits(emu, how):
    law = (np.array([0.5, 0.0, 2.0]), np.full(3, MU[0]), np.full(3, SIG[0]))
    outs, _, _, stat = run(emu, how, 50, 25, 3, 4, law, same=True, shared=True, snaps=[2, 4])
    outp, _, _, _ = run(emu, how, 50, 25, 3, 4, law, same=True, snaps=[2, 4])
    assert stat == 0 and np.array_equal(outs, outp)
    assert run(emu, how, 50, 25, 3, 2, law, same=False, shared=True, snaps=[2])[3] == 1  # a broken promise sets the word


@pytest.mark.parametrize("how", [4, 0], ids=["whole-loop", "streaming"])
def test_nine_groups_pick_their_matrix_sets(emu, how):
    """The batch of an eight-column Jacobian on 50x25 x 2: every group's samples against the reference at the group's parameters --
    group 5 on its own rebuilt v-grid, group 6 with lambda + eps, the groups 7 and 8 on the matrices of (mu + eps, sigma) and (mu,
    sigma + eps), which a difference of 1e-6 of a bump of 1e-2 would not tell apart: the bump here is 1e-2."""
    m1, m2, n0, N, eps, snaps = 50, 25, 2, 4, 1e-2, [2, 4]
    strikes, vs, _, ds, _, U0, spots = grids(m1, m2, n0)
    V_0 = Cm.v0_for(m2)
    lam, mu, sig = np.array([0.5, 0.0]), np.array([-0.10, 0.05]), np.array([0.15, 0.20])
    P, amp, top = BS.group_samples(m1, m2, snaps, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, V_0, vs, ds, U0, spots, None, lam, mu, sig, eps=eps)
    rows, v0s, lams = [], [], []
    for g in range(9):
        for k in range(n0):
            r = list(MODEL)  # rho, sigma, kappa, eta
            if 1 <= g <= 4:
                r[{1: 2, 2: 3, 3: 1, 4: 0}[g]] += eps
            rows.append(r + [Cm.T / N, N, 0.0, 0.0])
            v0s.append(V_0 + eps if g == 5 else V_0)
            lams.append(lam[k] + eps if g == 6 else lam[k])
    Gv = [O.rebuild_variance(m2, v) for v in v0s]
    vv, dv = np.ascontiguousarray(np.stack([g[0] for g in Gv])), np.ascontiguousarray(np.stack([g[1] for g in Gv]))
    musig = [[mu[k] + (eps if s == 1 else 0.0), sig[k] + (eps if s == 2 else 0.0)] for s in range(3) for k in range(n0)]
    out, _, _, _ = launch(emu, how, m1, m2, n0, np.array(rows), np.ascontiguousarray(np.tile(vs, (9, 1))), vv,
                          np.ascontiguousarray(np.tile(ds, (9, 1))), dv, U0, lams, musig, 3, False, V_0, v0s, spots, None, snaps)
    out = out.reshape(9, n0, len(snaps), -1)
    for g in range(9):
        within_bound("group %d" % g, out[g], (P[g], amp, top))
    assert np.array_equal(out[7, 1], out[0, 1]) and np.array_equal(out[8, 1], out[0, 1])  # lambda = 0: skipped as its group 0 is
    assert np.abs(out[7, 0] - out[0, 0]).max() > 1e-4 and np.abs(out[8, 0] - out[0, 0]).max() > 1e-4 and np.abs(out[6] - out[0]).min() >= 0.0


# ---- the route ----------------------------------------------------------------------------------------------------------------------
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING, SMALL_JUMP = range(7)  # enum HadiRouteKind
TH = {0: Cm.THETA, 1: 0.5, 2: 1.0 / 3.0, 3: 0.5 + 3.0 ** 0.5 / 6.0}
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
LOOP_WORDS = "; Bates: jump sub-step on the fp64 matrix core inside the time loop"


def route(emu, n, m1, m2, jumps, n_snap=0, n_samp=0, variant=0, scheme=0, tuning="", prec=0, profiling=0, debug=0):
    arr = (C.c_int * 16)(256, n, m1, m2, variant, scheme, prec, 0, debug, profiling, n_snap, int(variant == 2), 1, 0, 0, 0)
    o, desc = (C.c_longlong * 16)(), C.create_string_buffer(1024)
    emu.emu_route_bates_samples.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    assert emu.emu_route_bates_samples(arr, TH[scheme], tuning.encode(), int(jumps), n_samp, o, desc, 1024) == 0
    return list(o), desc.value.decode()


def test_jumps_without_samples_still_stream(emu):
    """Every case of tests/test_emu_jumps.py::test_route_is_always_streaming, whatever "jump_small" says."""
    cases = [(3, 50, 25, 0, "", SMALL), (300, 50, 25, 0, "", SMALL_SEQ), (600, 50, 25, 0, "", SMALL_SEQ2),
             (3, 50, 25, 0, "small_seq=1,small_pairs=1", SMALL_SEQ2), (300, 50, 25, 2, "", SMALL_SCH), (3, 50, 25, 2, "small_sch=1", SMALL_SCH),
             (20, 300, 80, 0, "", STREAMING), (4, 300, 140, 0, "", TEAM)]
    for js in ("", "jump_small=1", "jump_small=0"):
        for n, m1, m2, scheme, tuning, kind in cases:
            t = ",".join(x for x in (tuning, js) if x)
            o0, d0 = route(emu, n, m1, m2, False, scheme=scheme, tuning=t)
            o1, d1 = route(emu, n, m1, m2, True, scheme=scheme, tuning=t)
            assert o0[1] == kind and o0[15] == 0 and "Bates" not in d0, (n, m1, m2, o0)
            assert o1[1] == STREAMING and o1[15] == 1 and o1[10] == 1 and d1.endswith(JUMP_WORDS) and "row pass" in d1, d1
            # a ladder without samples (no such entry point, but the route function takes it): streams as well
            o2, d2 = route(emu, n, m1, m2, True, n_snap=3, scheme=scheme, tuning=t)
            assert o2[1] == STREAMING and d2.endswith(JUMP_WORDS) and "maturity ladder" in d2, d2


def test_jumps_with_samples_follow_jump_small(emu):
    samp = "; sampled ladder: 3 snapshots x 10 samples evaluated inside the time loop"
    for n, W in ((1, 8), (9, 8), (255, 8), (256, 8), (512, 8), (513, 4), (3000, 4)):
        o, d = route(emu, n, 50, 25, True, n_snap=3, n_samp=10, tuning="jump_small=1")
        assert o[1] == SMALL_JUMP and o[2] == W and o[15] == 1 and o[10] == 0, (n, o)  # (no U_temp: the copy lives in LDS)
        assert d.startswith("hadi_small_jump_kernel<1,%d>: whole time loop in one launch, instance resident in LDS (" % W) and d.endswith(samp + LOOP_WORDS), d
        o, d = route(emu, n, 50, 25, True, n_snap=3, n_samp=10, tuning="jump_small=0")
        assert o[1] == STREAMING and o[10] == 1 and d.endswith(JUMP_WORDS) and "hadi_sample_kernel after each snapshot step" in d, d
        o, d = route(emu, n, 50, 25, True, n_snap=3, n_samp=10)  # automatic: from one instance per CU on (profiles/bates_surface_ab.txt)
        assert o[1] == (SMALL_JUMP if n >= 256 else STREAMING), (n, o)
    o, d = route(emu, 2, 100, 12, True, n_snap=2, n_samp=4, variant=2, tuning="jump_small=1")  # B = 2, dividends
    assert o[1] == SMALL_JUMP and d.startswith("hadi_small_jump_kernel<2,8>"), d
    # all weights zero: the plain sample call, on whatever route that takes, with its words
    for n, kind in ((3, SMALL), (300, SMALL_SEQ)):
        o, d = route(emu, n, 50, 25, False, n_snap=3, n_samp=10, tuning="jump_small=1")
        assert o[1] == kind and "Bates" not in d and d.endswith(samp), d


def test_refused_shapes_stream(emu):
    kw = dict(n_snap=3, n_samp=10)
    for what in (dict(scheme=2), dict(tuning="jump_small=1,small_grid=0"), dict(tuning="jump_small=1,strip=0"),
                 dict(tuning="jump_small=1,row_tile=4"), dict(tuning="jump_small=1", profiling=1)):
        t = what.pop("tuning", "jump_small=1")
        o, d = route(emu, 3, 50, 25, True, tuning=t, **kw, **what)
        assert o[1] == STREAMING and o[15] == 1 and "hadi_small_jump_kernel" not in d and d.endswith(JUMP_WORDS), (what, d)
    for m1, m2 in ((300, 20), (200, 40), (128, 64)):  # grids the block kernel does not admit
        o, d = route(emu, 3, m1, m2, True, tuning="jump_small=1", **kw)
        assert o[1] == STREAMING and d.endswith(JUMP_WORDS), (m1, m2, d)
