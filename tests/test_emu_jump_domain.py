"""CPU-only: ONE launch of the Bates sub-step under the wave emulator (tests/emu/emu_jump_substep.cpp) over its admitted domain,
judged in isolation by the rule of tests/jump_cases.py -- a rough field, the kernel's own matrix, the product in np.longdouble and
the derived bound of a K-term inner product.  Around it: no pad slot, no slot beyond m1 and no identity row of the packed state
changes (they hold NaN in front of the launch, so whatever the kernel reads of them shows in the result); instances outside the
launched sub-range, finished instances and instances of weight 0 keep their bits.

Shapes: every m1 and m2 edge of tests/jump_cases.py (m1 >= 512 with 5 rows and two instances, to keep a case to seconds); launches
that start at instance o in {0, 1, n_src - 1, n_src + 1} of a batch of 6 n_src (hadi_jump_kernel: the five-column Jacobian's batch)
and 9 n_src (hadi_jump_sel_kernel: the eight-column one, also as the halves 14 + 13 of 27 that two streams cut it into), 1, 3 and 8
instances per block, strips shared by the set-0 instances of a source with cap 1, 3 and 7.  Every matrix of a batch has its own law,
so a wrong pick is a wrong product.  The matrices are held to the numpy generator on the rows of the table at every edge width.

Mutations, each applied by hand to a scratch copy of csrc/hadi_k_jumps.h (never committed) and run against the emulator tests of the
sub-step; "old" = tests/test_emu_jumps.py + tests/test_emu_jumps8.py, "new" = this file:

    mutation                                                        old tests fail          new tests fail
    last K tile dropped (ntile - 1)                                 12 (every_layout, mixed,  89: every m1 and m2 edge, every sub-range launch
                                                                     ring_and_strips)        of both kernels, shared, the self-test
    ok1 taken from i0 (fetch's second mask)                         none                    89: the same (a pad's NaN reaches a node, or a
                                                                                             node beside a pad is dropped)
    `sl & 3` order reversed (hadi_jump_entry)                       30 (every sweep test)   91: the same and the wide-law sweeps
    HADI_JUMP_UP 34 -> 32                                           none                    1: the_pitch_of_the_staged_tile_... (no result
                                                                                             depends on the pitch -- every product test
                                                                                             passes with the same bits -- so the property
                                                                                             the pitch exists for is asserted as arithmetic
                                                                                             on the constant)
    matrix pick without inst0, hadi_jump_kernel                     none                    9: jump_kernel_on_a_sub_range, o = 1, 2, 4
    matrix pick without inst0, hadi_jump_sel_kernel                 4 (jumps8: lists, two   29: jump_sel_kernel_on_a_sub_range (every range
                                                                     wavefronts)             with o > 0), other_layouts
    entries below 1e-9 zeroed (hadi_jump_matrix_kernel)             35 (the matrix test     19: the matrix at 17 of the 19 edge widths, both
                                                                     and every sweep test)   ill-grid matrix tests (the product tests use
                                                                                             the kernel's own matrix and rightly pass)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import jump_cases as JC
import jumps_ref as JR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_jump_substep.so")
_dp = C.POINTER(C.c_double)


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in os.listdir(os.path.join(HERE, "emu")) if f.endswith((".cpp", ".h"))] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp,
                               os.path.join(HERE, "emu", "emu_jump_substep.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_jump_substep_layout.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def substep(emu, kernel, m1, m2, vs_mat, musig, U, avec, o, cnt, n_src, width, shared=False, per=0, share=0, done=None):
    """One launch -> (U_out [n][m], G [n_mat][m1+1][m1+1]); the invariants of the packed state are asserted here."""
    n, n_mat = U.shape[0], vs_mat.shape[0]
    lay = (C.c_longlong * 10)()
    size = emu.emu_jump_substep_layout(n, m1, m2, lay)
    assert size > 0 and lay[4] == JC.k_extent(m1) and (lay[6], lay[7]) == JC.pick_shape(m1), list(lay)
    P0, P1, pad = np.zeros(size), np.zeros(size), np.zeros(size, dtype=np.uint8)
    Uout, G = np.zeros_like(U), np.full((n_mat, m1 + 1, m1 + 1), np.nan)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    rc = emu.emu_jump_substep(kernel, n, m1, m2, n_mat, _P(np.ascontiguousarray(vs_mat)), _P(np.ascontiguousarray(musig)), _P(U),
                              _P(np.ascontiguousarray(avec)), None if dn is None else dn.ctypes.data_as(C.c_void_p), o, cnt, n_src, width,
                              int(shared), per, share, C.c_double(np.nan), _P(P0), _P(P1), pad.ctypes.data_as(C.c_void_p), _P(Uout), _P(G))
    assert rc == 0, rc
    pad = pad.astype(bool)
    stride = size // n
    assert pad.any() and np.isnan(P0[pad]).all() and np.isfinite(P0[~pad]).all()
    assert np.array_equal(bits(P1)[pad], bits(P0)[pad]), "a pad slot, a slot beyond m1 or an identity row changed"
    outside = np.ones(size, dtype=bool)
    outside[o * stride:(o + cnt) * stride] = False
    assert np.array_equal(bits(P1)[outside], bits(P0)[outside]), "an instance outside the launch changed"
    assert np.isfinite(P1[~pad]).all(), "a node took up a pad's NaN"
    for k in range(n):
        if not o <= k < o + cnt or avec[k] == 0.0 or (done is not None and done[k]):
            assert np.array_equal(bits(Uout[k]), bits(U[k])), "instance %d must keep its bits" % k
    assert np.isfinite(G).all() and not G[:, 0].any()
    return Uout, G


def judge(name, m1, m2, U, Uout, G, mat_of, avec, live):
    worst = 0.0
    for k in live:
        r, at = JC.substep_ratio(U[k], Uout[k], G[mat_of(k)], avec[k], m1, m2)
        assert not np.array_equal(Uout[k], U[k])
        worst = max(worst, r)
        assert r <= 1.0, (name, k, r, at)
    print("%s %dx%d: worst |D - R| at %.3f of its bound" % (name, m1, m2, worst))
    return worst


def plain_batch(m1, m2, n, n_src, seed, pool=JC.DENSE + JC.MILD):
    """n instances over n_src grids and laws (instance k on grid and matrix k % n_src), rough fields, weights 1 and 0.37."""
    vs, _ = JC.s_grids(m1, n_src)
    mu, sg = JC.laws_for(n_src, pool=pool)
    U = JC.rough_field(seed, vs[np.arange(n) % n_src], m2)
    avec = np.array([JC.WEIGHTS[k % 2] for k in range(n)])
    return vs, np.ascontiguousarray(np.stack([mu, sg], axis=1)), U, avec


def test_the_pitch_of_the_staged_tile_spreads_a_half_wave_over_32_banks(emu):
    """What HADI_JUMP_UP is for, as arithmetic on the constant (no result depends on it, so no product test can see it): the A operand
    of one matrix instruction is read by lane 16 k + j at double (16 wave + j) UP + k (+ 4 kk); the 16 rows x 2 k-columns of a
    half-wave must fall on 32 different 8-byte banks.  The pitch holds a whole tile, and is even: the tile is written as double2."""
    lay = (C.c_longlong * 10)()
    assert emu.emu_jump_substep_layout(1, 50, 12, lay) > 0
    up, kc = lay[8], lay[9]
    assert up >= kc and up % 2 == 0 and kc == 32
    for half in (0, 1):
        banks = {((lane & 15) * up + (lane >> 4)) % 32 for lane in range(32 * half, 32 * half + 32)}
        assert len(banks) == 32, (up, sorted(banks))


# ---- every width and every row count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", JC.M1_EDGES)
def test_every_m1_edge(emu, m1):
    """A batch of 3 (2 from m1 = 512 on) with its own grid and dense law per instance; the field is rough (asserted)."""
    m2, n = (JC.M1_M2, 3) if m1 < 512 else (4, 2)
    vs, musig, U, avec = plain_batch(m1, m2, n, n, seed=m1)
    assert all(JC.roughness(U[k], m1, m2) >= 0.1 for k in range(n)) or m1 < 3
    Uout, G = substep(emu, 0, m1, m2, vs, musig, U, avec, 0, n, n, 1)
    judge("m1 edge", m1, m2, U, Uout, G, lambda k: k, avec, range(n))


@pytest.mark.parametrize("m2", JC.M2_EDGES)
def test_every_m2_edge(emu, m2):
    m1, n = JC.M2_M1, 3
    vs, musig, U, avec = plain_batch(m1, m2, n, n, seed=1000 + m2)
    assert all(JC.roughness(U[k], m1, m2) >= 0.1 for k in range(n))
    Uout, G = substep(emu, 0, m1, m2, vs, musig, U, avec, 0, n, n, 1)
    judge("m2 edge", m1, m2, U, Uout, G, lambda k: k, avec, range(n))


@pytest.mark.parametrize("m1", [50, 300, 600])
def test_shared_matrix_with_several_instances_per_block(emu, m1):
    """g_stride 0: one staged strip serves 3 instances of a block; the last block of the launch holds one."""
    m2, n = (12, 7) if m1 < 512 else (4, 4)
    vs, _ = JC.s_grids(m1, n, same=True)
    U = JC.rough_field(7 + m1, vs, m2)
    avec = np.array([JC.WEIGHTS[k % 2] for k in range(n)])
    avec[2] = 0.0
    musig = np.array([JC.DENSE[0]])
    Uout, G = substep(emu, 0, m1, m2, vs[:1], musig, U, avec, 0, n, n, 3, shared=True)
    judge("shared", m1, m2, U, Uout, G, lambda k: 0, avec, [k for k in range(n) if avec[k] != 0.0])


# ---- the teeth of the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2", [(50, 12), (300, 12), (1024, 4)])
def test_the_rule_sees_one_entry_moved_by_1e_9(emu, m1, m2):
    """Reference-side self-test: one entry of G_dev moved by 1e-9 of its row's max|G| before R is formed -- a near pair, a far pair and
    one in the last K tile that holds a node -- makes the check fail; unperturbed it passes."""
    n = 1
    vs, musig, U, avec = plain_batch(m1, m2, n, n, seed=5)
    avec[0] = 1.0
    Uout, G = substep(emu, 0, m1, m2, vs, musig, U, avec, 0, n, n, 1)
    assert JC.substep_ratio(U[0], Uout[0], G[0], 1.0, m1, m2)[0] <= 1.0
    for name, (i, l) in JC.teeth_positions(m1).items():
        r, at = JC.substep_ratio(U[0], Uout[0], G[0], 1.0, m1, m2, perturb=(i, l, 1e-9))
        print("m1 = %d, %s (%d, %d): %.1f of the bound at %s" % (m1, name, i, l, r, at))
        assert r > 1.0 and at[1] == i, (name, r, at)


# ---- launches that do not start at instance 0 ------------------------------------------------------------------------------------------
N_SRC = 3


@pytest.mark.parametrize("ipg", [1, 3, 8])
@pytest.mark.parametrize("o", [0, 1, N_SRC - 1, N_SRC + 1])
def test_jump_kernel_on_a_sub_range(emu, o, ipg):
    """hadi_jump_kernel over [o, o + 7) of 6 n_src = 18 instances: instance k of the BATCH multiplies with matrix k % n_src (three
    grids, three laws), whatever the launch's first instance; one instance of the range has finished, one has weight 0."""
    m1, m2, n, cnt = 50, 12, 6 * N_SRC, 7
    vs, musig, U, avec = plain_batch(m1, m2, n, N_SRC, seed=40 + o)
    done = np.zeros(n, dtype=np.int32)
    done[o + 2] = 1
    avec[o + 4] = 0.0
    Uout, G = substep(emu, 0, m1, m2, vs, musig, U, avec, o, cnt, N_SRC, ipg, done=done)
    live = [k for k in range(o, o + cnt) if k not in (o + 2, o + 4)]
    judge("o = %d, ipg = %d" % (o, ipg), m1, m2, U, Uout, G, lambda k: k % N_SRC, avec, live)
    # the teeth of THIS test: with the launch's own numbering the matrix would be (k - o) % n_src
    if o % N_SRC:
        assert JC.substep_ratio(U[o], Uout[o], G[0], avec[o], m1, m2)[0] > 1.0


def sel_batch(m1, m2, per, seed):
    """The nine groups of N_SRC sources: 3 per matrices, every one with its own law (the dense ones among them)."""
    n = 9 * N_SRC
    vs, _ = JC.s_grids(m1, N_SRC, same=(per == 1))
    pool = JC.DENSE + JC.MILD + ((-0.3, 0.4), (0.2, 0.6), (-0.5, 0.8))
    mu, sg = JC.laws_for(3 * per, pool=pool)
    U = JC.rough_field(seed, vs[np.arange(n) % N_SRC], m2)
    avec = np.array([JC.WEIGHTS[(k + k // N_SRC) % 2] for k in range(n)])
    vs_mat = vs[np.arange(3 * per) % N_SRC]
    mat_of = lambda k: (0 if k // N_SRC <= 6 else k // N_SRC - 6) * per + (k % N_SRC if per > 1 else 0)
    return n, vs_mat, np.ascontiguousarray(np.stack([mu, sg], axis=1)), U, avec, mat_of


SEL_RANGES = [(0, 27), (0, 14), (14, 13), (1, 20), (N_SRC - 1, 9), (N_SRC + 1, 22), (19, 8)]


@pytest.mark.parametrize("share,cap", [(0, 1), (0, 3), (1, 1), (1, 3), (1, 7)])
@pytest.mark.parametrize("o,cnt", SEL_RANGES, ids=["%d+%d" % r for r in SEL_RANGES])
def test_jump_sel_kernel_on_a_sub_range(emu, o, cnt, share, cap):
    """hadi_jump_sel_kernel over a sub-range of 9 n_src = 27 instances with per-source matrices: the whole batch, the halves 14 + 13
    of two streams, and ranges that start at 1, n_src - 1, n_src + 1 and inside group 6."""
    m1, m2 = 50, 12
    n, vs_mat, musig, U, avec, mat_of = sel_batch(m1, m2, N_SRC, seed=90 + o)
    done = np.zeros(n, dtype=np.int32)
    done[o + 3] = 1
    avec[o + 5] = 0.0
    Uout, G = substep(emu, 1, m1, m2, vs_mat, musig, U, avec, o, cnt, N_SRC, cap, per=N_SRC, share=share, done=done)
    live = [k for k in range(o, o + cnt) if k not in (o + 3, o + 5)]
    judge("sel [%d, %d) share %d cap %d" % (o, o + cnt, share, cap), m1, m2, U, Uout, G, mat_of, avec, live)


@pytest.mark.parametrize("m1,o,cnt,per,share,cap", [(65, 14, 13, N_SRC, 1, 7), (300, 0, 14, N_SRC, 1, 3), (513, 14, 13, N_SRC, 0, 1),
                                                    (300, 14, 13, 1, 0, 3), (50, 4, 20, 1, 0, 8)])
def test_jump_sel_kernel_on_other_layouts_and_shared_sets(emu, m1, o, cnt, per, share, cap):
    m2 = 12 if m1 < 512 else 4
    n, vs_mat, musig, U, avec, mat_of = sel_batch(m1, m2, per, seed=m1 + o)
    Uout, G = substep(emu, 1, m1, m2, vs_mat, musig, U, avec, o, cnt, N_SRC, cap, per=per, share=share)
    judge("sel %d [%d, %d) per %d share %d cap %d" % (m1, o, o + cnt, per, share, cap), m1, m2, U, Uout, G, mat_of, avec, range(o, o + cnt))


# ---- the matrix at every edge width -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", JC.M1_EDGES)
def test_matrix_kernel_against_the_numpy_generator_at_every_edge(emu, m1):
    """hadi_jump_matrix_kernel, all rows, against tests/jumps_ref.py (which tests/test_jumps_exact.py holds to 40 digits) at the
    entry bound, on a well-conditioned grid (asserted) and the laws of the table -- above m1 = 129 the densest and the narrowest law only."""
    K = Cm.well_conditioned_strikes(m1, 1)[0]
    g = O.grid(m1, 8 * K, Cm.S_0, K, K / 5, 8, 5.0, Cm.V_0, 5.0 / 500)
    vs = g[0]
    assert Cm.interval_ratios(g[2])[0] <= Cm.COND_MAX
    for mu, sig in (JC.LAWS if m1 <= 129 else (JC.LAWS[2], JC.LAWS[5])):
        G = np.full((m1 + 1, m1 + 1), np.nan)
        assert emu.emu_jump_matrix(m1, _P(vs), C.c_double(mu), C.c_double(sig), _P(G)) == 0
        worst = (np.abs(G - JR.generator(vs, mu, sig)) / JC.entry_bound(vs, mu, sig)[:, None]).max()
        print("m1 = %d (%g, %g): worst entry at %.3f of its bound" % (m1, mu, sig, worst))
        assert np.isfinite(G).all() and worst <= 1.0 and not G[0].any()


@pytest.mark.parametrize("m1,m2", JC.ILL_SHAPES)
def test_matrix_kernel_on_ill_conditioned_s_grids(emu, m1, m2):
    """Every placement of the tiny interval (R = 1e6): entries row by row at max(entry bound, 30 x the numpy formula's own recorded
    distance from 40 digits), the two-column sum, the action on the payoffs and the row sums (jump_cases.ill_matrix_check)."""
    import json
    places, K = JC.ill_s_grids(m1)
    fix = json.load(open(os.path.join(HERE, "golden", JC.ILL_FIXTURE)))["cases"]
    worst = np.zeros(4)
    for name, vs, ds, tiny in places:
        for law in (JC.ILL_LAWS if m1 <= 129 else JC.ILL_LAWS[:1]):
            rec = fix[JC.ill_key(m1, name, law)]
            assert rec["rows"] == JC.ill_rows(m1, tiny) and rec["tiny"] == tiny
            G = np.full((m1 + 1, m1 + 1), np.nan)
            assert emu.emu_jump_matrix(m1, _P(np.ascontiguousarray(vs)), C.c_double(law[0]), C.c_double(law[1]), _P(G)) == 0
            worst = np.maximum(worst, JC.ill_matrix_check("m1 = %d, %s" % (m1, name), G, vs, K, tiny, law, rec))
    print("m1 = %d: worst margins (entries, sum, action, row sums) %s" % (m1, worst))
    assert (worst <= 1.0).all(), worst


# ---- wide laws over several steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2", [(50, 25), (300, 12)])
def test_wide_laws_over_four_steps(emu, m1, m2):
    """The dense laws behind the emulated streaming kernels against tests/jumps_ref.py at the family's 1e-10, N = 4.  The intensity
    keeps a |kbar| max(s_i / h_i) <= 1 (asserted on the inputs): beyond it the explicit compensator amplifies round-off and the
    comparison means nothing."""
    import test_emu_jumps as TE
    n, N = 3, 4
    vs = TE.grids(m1, m2, n)[1]
    mu, sig = JC.laws_for(n, pool=JC.DENSE)
    dt = TE.Cm.T / N
    lam = np.array([JC.stable_intensity(vs[k], mu[k], sig[k], dt) for k in range(n)])
    for k in range(n):
        assert lam[k] * dt * abs(JR.kbar(mu[k], sig[k])) * JC.stiffness(vs[k]) <= 1.0
    TE.check(emu, "wide laws", m1, m2, n, *TE.uniform(n, N), (lam, mu, sig))
