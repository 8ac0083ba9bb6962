"""CPU-only check of the KERNEL SOURCE (csrc/hadi_kernels.h, csrc/hadi_core.h) compiled with g++ against
the test-only wave emulator in tests/emu: same code, host threads instead of wavefronts.  This is a
development safety net for layout / indexing / table logic; it proves nothing about the GPU build,
whose parity tests are the `-m gpu` ones."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu.so")
_dp = C.POINTER(C.c_double)


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", EMU_SO,
                               os.path.join(HERE, "emu", "emu_driver.cpp")])
    return C.CDLL(EMU_SO)


def _run(emu, m1, m2, N, strikes, variant, target_waves, r_f=0.0, small=0, scheme=0, put=False, tol=1e-11, divs=Cm.DIVS):
    """scheme: 0 Douglas, 1 Craig-Sneyd, 2 Douglas with the state kept in fp32 between the passes, 3 Douglas with the
    American P representation (no lambda_bar array; explicit pair on step 1 and on dividend steps).  divs: the dividend
    schedule (dates, amounts, percentages) of the DIV / AM_DIV variants, for the emulator and for the oracle."""
    n = len(strikes)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes)
    ks = np.array(strikes, dtype=np.float64)
    if put:
        U0 = np.ascontiguousarray(np.tile(np.maximum(ks[:, None] - vs, 0.0), (1, m2 + 1)))
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, variant,
                      divs if variant in (O.DIV, O.AM_DIV) else None, option_type=O.PUT if put else O.CALL, strikes=ks if put else None)
    p.scheme = 1 if scheme == 1 else 0
    p.state_fp32 = 1 if scheme == 2 else 0
    Uo, lamo, _ = O.solve_batch(p, vs, vv, ds, dv, U0, U0, want_lambda=True)
    assert np.isfinite(Uo).all()
    U, lam = U0.copy(), np.zeros_like(U0)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (n, 1)).copy()
    dd = [np.array(x, dtype=np.float64) for x in divs]
    rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D),
                       C.c_double(r_f), _P(par), variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam),
                       target_waves, len(dd[0]), _P(dd[0]), _P(dd[1]), _P(dd[2]), 64, small, scheme, _P(ks) if put else None,
                       None, None)
    assert rc == 0
    scale = np.abs(Uo).max()
    # fp32 state: an fp64 last-bit difference before a store can flip the float rounding (6e-8 relative), per step
    assert np.abs(U - Uo).max() < (2e-7 * N if scheme == 2 else tol) * scale
    if lamo is not None:
        assert np.abs(lam - lamo).max() < 1e-9 * max(1.0, np.abs(lamo).max())


def test_row_pass_one_node_per_lane_and_r_f(emu):
    _run(emu, 40, 12, 3, [90.0, 110.0], O.EU, 8, r_f=0.01)


def test_row_pass_two_nodes_per_lane(emu):
    _run(emu, 100, 20, 2, [100.0], O.EU, 8)


def test_american_projection(emu):
    _run(emu, 40, 12, 3, [100.0], O.AM, 4)


def test_dividends_and_chunked_column_pass(emu):
    # m2 = 70 -> 71 v-rows -> two chunks coupled by the SPIKE reduced system; dividend lands on step 2
    _run(emu, 72, 70, 6, [100.0], O.DIV, 3)


def test_single_buffer_column_pass_for_more_than_8_chunks(emu):
    # m2 = 270 -> 271 v-rows -> 9 chunks -> the 16-wave single-buffer kernel; few blocks per instance so that a block
    # walks several column tiles (store + reload of the same registers), American adds the projection
    _run(emu, 70, 265, 1, [97.0], O.AM, 1, r_f=0.01)
    # European sweeps: hadi_pass_b2 (12 rows of the next tile prefetched into LDS, 24 with the fp32 state; one exchange buffer)
    # and, with the prefetch switched off, hadi_pass_b1; 9 and 16 chunks, a short last tile, a block of one tile
    for pf in (1, 0):
        emu.emu_set_tuning(b"col_prefetch", pf)
        emu.emu_set_tuning(b"tile_interleave", pf)  # (with it: the blocks take their full tiles interleaved)
        try:
            _run(emu, 100, 270, 1, [100.0], O.EU, 1)
            if pf:
                _run(emu, 64, 500, 1, [100.0], O.EU, 8, r_f=0.01)      # 16 chunks (1024-thread block), two tiles
                _run(emu, 100, 270, 1, [100.0], O.EU, 1, scheme=2)     # fp32 state: 16 rows prefetched, 4 rows per DMA instruction
        finally:
            emu.emu_set_tuning(b"reset", 0)


def test_strip_row_pass(emu):
    # 8 nodes per lane: every wavefront walks a strip of v-rows alone (register window + private LDS ring, no barrier).
    # 151 rows -> 8 strips of 19; r_f != 0 exercises the boundary terms, the last strip carries the b2 row
    _run(emu, 300, 150, 1, [100.0], O.EU, 1, r_f=0.01)
    # forced short strips (6 rows: prologue / halo / ring wrap-around on every strip), American adds lambda_bar
    emu.emu_set_tuning(b"strip", 1)
    try:
        _run(emu, 280, 40, 2, [95.0], O.AM, 1)
        # 4 and 2 nodes per lane
        _run(emu, 200, 60, 3, [100.0], O.AM_DIV, 1, r_f=0.01)
        _run(emu, 100, 70, 2, [100.0], O.EU, 1)
        # put boundary data on strips (i = 0 column with its reaction term, b1 == 0, time factor e^{-r_d t})
        _run(emu, 300, 40, 2, [100.0], O.AM, 1, put=True)
    finally:
        emu.emu_set_tuning(b"reset", 0)


def test_put_boundary_data(emu):
    # not a reference feature (hadi.h, enum hadi_option_type): shared-ring kernel at 1 and 4 nodes per lane, the LDS-resident
    # small-grid kernel, dividends (ex-dividend spot <= 0 takes the s = 0 value), American projection, two waves per row
    _run(emu, 40, 12, 3, [90.0, 110.0], O.EU, 8, put=True)
    _run(emu, 40, 12, 4, [100.0], O.AM_DIV, 8, small=1, put=True)
    _run(emu, 200, 40, 6, [100.0], O.AM_DIV, 8, put=True)
    _run(emu, 600, 12, 2, [100.0], O.EU, 8, put=True)


def test_more_v_nodes_than_s_nodes(emu):
    # m2 > m1: the b1 quirk index m1*(j+1) then puts TWO entries on the v-rows k*m1 (columns 0 and m1)
    _run(emu, 20, 50, 3, [100.0], O.EU, 8, r_f=0.01)
    _run(emu, 40, 70, 2, [100.0, 95.0], O.AM, 8, r_f=0.01)
    _run(emu, 70, 100, 2, [100.0], O.EU, 1, r_f=0.01)   # 2 nodes per lane; chunked column pass


def test_fp32_state_sweep(emu):
    # state stored as float between the passes (arithmetic fp64), against the oracle with the same two roundings per step:
    # one node per lane, 8 nodes per lane, two wavefronts per row, and the single-buffer column pass
    _run(emu, 40, 12, 3, [90.0, 110.0], O.EU, 8, r_f=0.01, scheme=2)
    _run(emu, 300, 40, 2, [100.0], O.EU, 8, scheme=2)
    _run(emu, 600, 12, 2, [100.0], O.EU, 8, scheme=2)
    _run(emu, 300, 150, 1, [100.0], O.EU, 1, r_f=0.01, scheme=2)  # large enough for the strip row pass (ring of floats)
    # (the single-buffer column pass with the fp32 state: test_single_buffer_column_pass_for_more_than_8_chunks)


def test_american_p_representation(emu):
    # one node per lane, 4 nodes per lane with dividends (explicit steps in between), two wavefronts per row,
    # the single-buffer column pass
    _run(emu, 40, 12, 4, [100.0, 92.0], O.AM, 4, r_f=0.01, scheme=3)
    _run(emu, 200, 33, 7, [100.0], O.AM_DIV, 8, scheme=3)
    _run(emu, 530, 10, 2, [100.0], O.AM, 8, scheme=3)
    _run(emu, 70, 265, 1, [97.0], O.AM, 1, scheme=3)
    # batches large enough for the strip row pass: 8 nodes per lane (payoff row in LDS), with dividend steps in between,
    # and 4-strip blocks at 2 nodes per lane
    _run(emu, 300, 70, 2, [100.0], O.AM, 1, r_f=0.01, scheme=3)
    _run(emu, 120, 40, 6, [95.0], O.AM_DIV, 1, scheme=3)


def test_two_waves_per_row_split_solve(emu):
    # m1 > 512: the row's tridiagonal system is split over two wavefronts and re-coupled by a 2x2 system
    _run(emu, 600, 12, 2, [100.0, 93.0], O.EU, 8)
    _run(emu, 530, 10, 2, [100.0], O.AM, 8, r_f=0.01)


def test_paired_strip_row_pass(emu):
    # 512 < m1 <= 1024 on barrier-free strips: a PAIR of wavefronts walks each strip, one half of the row each (own LDS-DMA
    # pieces, split tridiagonal solve with a 2x2 exchange and a pair rendezvous per row, the partner's boundary node carried
    # from the partner's half of the ring).  41 rows -> 4 strips of 11 (ascending and descending, the last one short and
    # carrying the b2 row); 3-slot ring (fp64 state) and 4-slot ring of floats (fp32 state); full width m1 = 1024; put data.
    emu.emu_set_tuning(b"strip", 1)
    try:
        _run(emu, 600, 26, 2, [100.0], O.EU, 1, r_f=0.01)
        _run(emu, 600, 26, 2, [100.0], O.EU, 1, scheme=2)  # fp32 state
        # American sweeps on paired strips (round 3): explicit (U, lambda_bar) pair, with dividends, put data; the P
        # representation (u0 carried raw, U = max(P, U_0) rebuilt inside the step; explicit steps in between for dividends)
        _run(emu, 530, 20, 2, [100.0], O.AM, 1)
        _run(emu, 700, 26, 4, [96.0], O.AM_DIV, 1, r_f=0.01, put=True)
        _run(emu, 1024, 20, 2, [100.0], O.AM, 1, scheme=3, put=True)
        _run(emu, 700, 26, 6, [104.0], O.AM_DIV, 1, scheme=3, r_f=0.01)
    finally:
        emu.emu_set_tuning(b"reset", 0)


def test_craig_sneyd_predictor_corrector(emu):
    # solver.hpp:781-907: Douglas predictor + corrector re-adding dt/2 (A0 Y2 - A0 U); r_f != 0 exercises the b terms
    _run(emu, 40, 12, 3, [100.0, 91.0], O.EU, 8, r_f=0.01, scheme=1)
    _run(emu, 100, 20, 2, [100.0], O.EU, 8, scheme=1)


def test_craig_sneyd_on_barrier_free_strips(emu):
    """Round 4: predictor (MODE 1: the Douglas strip step that also stores R1 and C2) and corrector (MODE 2: rows of Y2
    through the ring, the R1 / C2 rows of each step as register loads requested a step ahead) on
    hadi_pass_a_strip at 2, 4 and 8 nodes per lane and on paired strips (m1 > 512); strips with and without a partner,
    descending and ascending, the b2 row, r_f != 0 (b1 along the anti-diagonal), several instances.  The emulator checks
    arithmetic and indexing; the waits are what libhadi_strict.so checks on hardware."""
    emu.emu_set_tuning(b"strip", 1)
    try:
        _run(emu, 100, 20, 3, [100.0, 92.0], O.EU, 1, r_f=0.01, scheme=1)   # 2 nodes per lane; 21 rows: 4 strips of 6, the last one short
        _run(emu, 200, 26, 2, [100.0], O.EU, 1, scheme=1)                   # 4 nodes per lane
        _run(emu, 300, 34, 2, [104.0], O.EU, 1, r_f=0.02, scheme=1)         # 8 nodes per lane: 35 rows, 7 strips of 5 (one without a partner)
        _run(emu, 700, 20, 2, [100.0], O.EU, 1, r_f=0.01, scheme=1)         # paired strips
    finally:
        emu.emu_set_tuning(b"reset", 0)


def test_small_grid_lds_resident_kernel(emu):
    # whole instance in LDS, one launch for the time loop: all four variants on the reference's 50x25 grid
    _run(emu, 50, 25, 6, [100.0, 95.0], O.EU, 8, small=1)
    _run(emu, 50, 25, 12, [100.0], O.AM_DIV, 8, small=1)
    _run(emu, 100, 30, 4, [100.0], O.AM, 8, r_f=0.01, small=1)
    _run(emu, 40, 12, 12, [100.0], O.DIV, 8, small=1)
    # 8 wavefronts per instance (small batches)
    _run(emu, 50, 25, 6, [100.0], O.AM_DIV, 8, small=2)
    _run(emu, 100, 30, 3, [96.0], O.EU, 8, r_f=0.01, small=2)


def test_small_grid_sequential_kernel(emu):
    # European / dividend sweeps of LDS-resident grids: one wavefront per instance, lane <-> v-row in the row pass (sequential
    # Thomas, c' parked in the consumed columns of U), lane <-> s-column in the column pass.  One and two nodes per lane in
    # the packed layout (m1 <= 64 / <= 128), r_f != 0, dividends, put data, more v-nodes than s-nodes, two column rounds.
    _run(emu, 50, 25, 3, [100.0, 91.0], O.EU, 8, small=3)
    _run(emu, 50, 25, 12, [100.0], O.DIV, 8, r_f=0.01, small=3)
    _run(emu, 100, 30, 2, [96.0], O.EU, 8, r_f=0.01, small=3)
    _run(emu, 64, 32, 2, [100.0], O.EU, 8, small=3)
    _run(emu, 20, 25, 3, [100.0], O.EU, 8, r_f=0.02, small=3)
    _run(emu, 40, 12, 12, [105.0], O.DIV, 8, small=3, put=True)
    # two instances per wavefront (hadi_small_seq2_kernel): lanes 0..31 / 32..63 walk the v-rows of two instances through one
    # instruction stream; an odd batch (the last wavefront carries one instance), dividends, put data, r_f != 0, 32 v-rows
    _run(emu, 50, 25, 3, [100.0, 91.0, 104.0], O.EU, 8, small=5)
    _run(emu, 100, 31, 2, [96.0, 101.0], O.EU, 8, r_f=0.01, small=5)
    _run(emu, 40, 12, 12, [105.0, 95.0], O.DIV, 8, r_f=0.01, small=5, put=True)


def test_plan_invariants_over_shapes_and_batch_sizes(emu):
    """Host logic (hadi_plan.h): for every supported shape and a range of batch sizes the launch geometry covers all rows,
    columns and instances, and every kernel's dynamic LDS fits the 160 KB of a CU (incl. the payoff row the American P
    representation adds to the row kernels)."""
    LDS = 160 * 1024
    o = (C.c_longlong * 26)()
    shapes = [(m1, m2) for m1 in (20, 50, 64, 65, 100, 128, 129, 200, 256, 257, 300, 400, 512, 513, 700, 1024)
              for m2 in (8, 25, 32, 33, 64, 66, 100, 128, 131, 132, 200, 256, 263, 264, 300, 512) if m2 <= m1]
    seen_strip = set()
    for m1, m2 in shapes:
        for n in (1, 3, 64, 160, 256, 300, 512, 1100, 4000):
            for tw in (8, 2048):  # emulator-sized and MI355X-sized (8 wavefronts x 256 CUs)
                assert emu.emu_plan_full(m1, m2, n, tw, o) == 0, (m1, m2, n)
                (B, G, rowp, P, nrows, npad, stride, W, NG, PD, R, ntiles, grid_a, smem_a, use_strip, RS, sblocks, grid_as,
                 smem_as, ctiles, btpw, bgroups, grid_b, smem_b, use_pairs, smem_pairs) = list(o)
                assert nrows == m2 + 1 and npad == 33 * P and npad >= nrows and stride == rowp * npad
                assert 64 * B * G >= m1 and rowp == 64 * B * G + (16 if B >= 4 else 8) and B in (1, 2, 4, 8) and G in (1, 2)
                assert R % W == 0 and R * ntiles >= nrows and grid_a * NG >= n * ntiles
                assert smem_a + rowp * 8 <= LDS
                nwv = 8 if B == 8 else 4
                if use_pairs:  # two strips per wavefront (hadi_pass_a_pairs): 8 strips per 4-wavefront block, chosen only
                    # where the launch keeps two blocks per CU and the strips 16 rows
                    assert B == 4 and G == 1 and use_strip and RS >= 16 and RS * 8 * sblocks >= nrows and grid_as >= n * sblocks
                    assert n * sblocks >= 2 * max(1, tw // 8) and smem_pairs <= LDS
                    seen_strip.add("pairs")
                elif B >= 2 and G == 1:  # strips can be forced for any of these (hadi_set_tuning "strip"), so check them all
                    assert RS * nwv * sblocks >= nrows and grid_as >= n * sblocks
                    assert smem_as + rowp * 8 <= LDS
                elif G == 2:  # paired strips: 4 pairs per block, 3 ring slots of doubles
                    if use_strip:
                        assert 8 <= RS <= 64 and RS * 4 * sblocks >= nrows and grid_as >= n * sblocks
                        assert smem_as == 4 * 3 * rowp * 8 + (4 * 64 * B * G + 4 * 16) * 8 and smem_as <= LDS
                        seen_strip.add(16)
                else:
                    assert not use_strip
                if use_strip and G == 1:
                    assert B in (2, 4, 8) and (8 if B == 8 else 16) <= RS <= 64
                    seen_strip.add(B)
                # column tiles: the blocks' ranges (hadi_pb_tile_range) partition [0, ctiles), none is empty
                assert ctiles * 64 >= rowp and btpw >= 1
                nfull, nxt = rowp // 64, 0
                for grp in range(bgroups):
                    t0 = min(grp * btpw, nfull)
                    t1 = ctiles if grp == bgroups - 1 else min(t0 + btpw, nfull)
                    assert t0 == nxt and t1 > t0, (m1, m2, n, btpw, bgroups, grp)
                    nxt = t1
                assert nxt == ctiles
                # ... and so do the tile lists the kernels walk (hadi_pb_tiles), consecutive and interleaved: every tile once,
                # the short tile last in its block, the blocks' loads differing by at most one full tile
                tl = (C.c_int * 64)()
                for il in (0, 1):
                    seen, sizes = [], []
                    for grp in range(bgroups):
                        k = emu.emu_col_tiles(m1, m2, n, tw, il, grp, tl)
                        assert k >= 1, (m1, m2, n, il, grp, k)
                        mine = list(tl[:k])
                        assert all(t < nfull for t in mine[:-1]) and mine == sorted(mine)
                        seen += mine
                        sizes.append(sum(1 for t in mine if t < nfull))
                    assert sorted(seen) == list(range(ctiles)), (m1, m2, n, il, seen)
                    if il:
                        full_sizes = [z for z in sizes if z]
                        assert max(full_sizes) - min(full_sizes) <= 1 if full_sizes else True
                if (m1, m2, n, tw) == (1024, 512, 64, 2048):  # config 5: 16 full tiles on 4 blocks, the short one appended
                    assert (btpw, bgroups) == (4, 4)
                assert grid_b == (n * bgroups + 7) // 8 * 8 and smem_b <= LDS and P <= 16
    assert seen_strip == {2, 4, 8, 16, "pairs"}
    assert emu.emu_plan_full(100, 101, 1, 8, o) == 0  # m2 > m1 is covered (two b1 entries on the v-rows k*m1)
    assert emu.emu_plan_full(1025, 100, 1, 8, o) == 0 and o[0] == 1 and o[1] == 17  # beyond 1024: natural order, sequential row pass
    assert emu.emu_plan_full(600, 528, 1, 8, o) == 0 and o[3] == 1 and o[5] == 529  # beyond 16 chunks: one chunk, sequential column pass


def test_automatic_two_stream_choice_follows_the_idle_rounds_of_the_row_pass(emu):
    """hadi_plan_row_idle: batches of 512x256 whose row pass fills whole rounds of the 256 CUs (64, 128, 256 instances: two
    streams measured 5 - 12 % SLOWER) stay on one stream, batches that leave a partial round idle (32, 96, 160, 192: two
    streams measured 3 - 22 % faster) are cut in two; config 3 and config 5 fill their rounds.  A function of (shape, batch
    size) alone -- no timing, no history."""
    emu.emu_plan_row_idle_ppm.restype = C.c_longlong
    idle = lambda m1, m2, n: emu.emu_plan_row_idle_ppm(m1, m2, n, 256) / 1e6
    for n in (64, 128, 256):
        assert idle(512, 256, n) < 0.04, (n, idle(512, 256, n))
    for n, want in ((160, 0.0625), (192, 0.25), (96, 0.25)):
        assert abs(idle(512, 256, n) - want) < 1e-6, (n, idle(512, 256, n))
    assert idle(512, 256, 32) == 0.0 and idle(512, 256, 24) == 0.0  # shared-ring row pass: no rounds of equal blocks, one stream
    assert idle(256, 128, 512) < 0.04   # config 3: 512 pair-strip blocks, two per CU
    assert idle(1024, 512, 64) < 0.04   # config 5: 256 paired-strip blocks
    assert idle(1024, 512, 48) >= 0.04  # ... three quarters of a round


def test_setup_tables_against_oracle_operators(emu):
    """The O(m1+m2) tables reproduce the reference's dense operators: apply them to a random field and
    compare with the oracle's A0U / A1U / A2U of step 1."""
    m1, m2, N = 70, 30, 10
    vs, vv, ds, dv, _ = Cm.oracle_grids(m1, m2, [100.0])
    rng = np.random.default_rng(3)
    U = rng.standard_normal((m2 + 1) * (m1 + 1))
    p = Cm.oracle_params(m1, m2, N, "EU")
    _, _, d = O.solve(p, vs[0], vv[0], ds[0], dv[0], U, U, dump_step=1)
    plan = (C.c_int * 6)()
    assert emu.emu_plan(m1, m2, 1, 8, plan) == 0
    B, rowp, Pn, G = plan[0], plan[1], plan[2], plan[5]
    nrows = m2 + 1
    scoef, b2row = np.zeros(4 * 64 * B * G), np.zeros(rowp)
    npad = Pn * 33  # HADI_LC rows per column-pass chunk
    rowc, a2i, pb, rinv = np.zeros(nrows * 16), np.zeros(5 * npad), np.zeros(npad * 12), np.zeros(16 * Pn * Pn)
    rc = emu.emu_tables(m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(0.0),
                        C.c_double(Cm.RHO), C.c_double(Cm.SIGMA), C.c_double(Cm.KAPPA), C.c_double(Cm.ETA),
                        _P(vs[0]), _P(vv[0]), _P(ds[0]), _P(dv[0]), 8, _P(scoef), _P(b2row), _P(rowc), _P(a2i),
                        _P(pb), _P(rinv))
    assert rc == 0
    rowc = rowc.reshape(nrows, 16)

    def pos(i):
        if i == 0:
            return 64 * B * G
        e = i - 1
        g, el = divmod(e, 64 * B)
        if B == 1:
            return 64 * g + el
        lane, r = divmod(el, B)
        return (r >> 1) * 128 * G + 128 * g + 2 * lane + (r & 1)

    sc = scoef.reshape(4, 64 * B * G)  # Bm, Bp, Dm, Dp; centre weights are -(m + p)
    Ug = U.reshape(m2 + 1, m1 + 1)
    A0 = np.zeros_like(Ug); A1 = np.zeros_like(Ug); A2 = np.zeros_like(Ug)
    for j in range(m2 + 1):
        v = rowc[j, 0]
        for i in range(1, m1 + 1):
            Bk = [sc[0, pos(i)], -(sc[0, pos(i)] + sc[1, pos(i)]), sc[1, pos(i)]]
            Dk = [sc[2, pos(i)], -(sc[2, pos(i)] + sc[3, pos(i)]), sc[3, pos(i)]]
            nb = lambda jj: [Ug[jj, i - 1], Ug[jj, i], Ug[jj, i + 1] if i + 1 <= m1 else 0.0]
            lo, mn, up = [v * Dk[k] + (Cm.R_D - Cm.R_F) * Bk[k] for k in range(3)]
            mn -= 0.5 * Cm.R_D
            u = nb(j)
            A1[j, i] = lo * u[0] + mn * u[1] + up * u[2]
            if 1 <= j <= m2 - 1:
                A0[j, i] = sum(rowc[j, 1 + l] * sum(Bk[k] * nb(j - 1 + l)[k] for k in range(3)) for l in range(3))
        for i in range(m1 + 1):
            for k, off in enumerate((-2, -1, 0, 1, 2)):
                if 0 <= j + off <= m2:
                    A2[j, i] += rowc[j, 4 + k] * Ug[j + off, i]
    scale = lambda x: max(1.0, np.abs(x).max())
    assert np.abs(A0.ravel() - d["A0U"]).max() < 1e-12 * scale(d["A0U"])
    assert np.abs(A1.ravel() - d["A1U"]).max() < 1e-12 * scale(d["A1U"])
    assert np.abs(A2.ravel() - d["A2U"]).max() < 1e-12 * scale(d["A2U"])
    # boundary vectors: b2 on the last v-row, b1 at index m1*(j+1) (quirk)
    b1 = np.zeros((m2 + 1) * (m1 + 1))
    for j in range(m2 + 1):
        if rowc[j, 10] >= 0:
            b1[j * (m1 + 1) + int(rowc[j, 10])] = rowc[j, 9]
    assert np.array_equal(b1, d["b1"])
    b2 = np.zeros_like(b1)
    b2[m2 * (m1 + 1):] = [b2row[pos(i)] for i in range(m1 + 1)]
    assert np.array_equal(b2, d["b2"])


def _fuzz_instance(seed, index, k, small=False):
    """Instance k of a recorded fuzz case (tests/fuzz_cases.py) as single-instance arrays."""
    import fuzz_cases as F
    c = F.case(seed, index, small=small)
    K = c["strikes"][k]
    vs, vv, ds, dv, U0 = Cm.oracle_grids(c["m1"], c["m2"], [K])
    return c, K, vs, vv, ds, dv, U0


def test_one_node_per_lane_line_solve_keeps_close_nodes_together(emu):
    """Regression, fuzz seed 5 case 279 (FUZZ_SMALL, round 2: 'BAD', field error 1.16e-7 on one instance): instance 101 has
    S_0 = 100 inserted 7.4e-6 beside a node of the 16-interval s-grid -- off-diagonals of 1e7 in I - theta dt A1.  With one
    node per lane the cyclic reduction is the whole line solve; its plain diagonal update 1 - a cL - c aR lost seven digits
    there and, worse, gave the two close nodes INDEPENDENT errors, which the next step multiplies by the 1e7 coupling.
    The extended-precision adjudicator (oracle/heston_oracle_xp.c) measured |libhadi - exact| = 1.7e-7 against 4.5e-10
    for the reference's Thomas sweep; with the excess-carrying update (hadi_row_step, NB == 0) libhadi is at the oracle's
    level.  All three kernels that run hadi_row_step<1>: streaming, LDS-resident with 4 and with 8 wavefronts."""
    c, K, vs, vv, ds, dv, U0 = _fuzz_instance(5, 279, 101, small=True)
    assert (c["m1"], c["m2"], c["N"], c["name"]) == (16, 11, 9, "AM_DIV") and ds.min() < 1e-5
    m1, m2, N = c["m1"], c["m2"], c["N"]
    par = np.array([c["model"]])
    dd = [np.array(x, dtype=np.float64) for x in Cm.DIVS]
    for variant in (O.AM_DIV, O.EU):
        p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, c["r_f"], *c["model"], variant,
                          Cm.DIVS if variant == O.AM_DIV else None)
        Uo, lo, _ = O.solve(p, vs[0], vv[0], ds[0], dv[0], U0[0], U0[0])
        Ux, lx = O.solve_xp(p, vs[0], vv[0], ds[0], dv[0], U0[0], U0[0])
        scale = np.abs(Ux).max()
        e_oracle = np.abs(Uo - Ux).max() / scale
        assert e_oracle < 2e-9  # the fp64 Thomas sweep itself: cond * eps
        for small in (0, 1, 2):
            U, lam = U0.copy(), np.zeros_like(U0)
            rc = emu.emu_solve(1, m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(c["r_f"]),
                               _P(par), variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), 8, len(dd[0]),
                               _P(dd[0]), _P(dd[1]), _P(dd[2]), 64, small, 0, None, None, None)
            assert rc == 0
            e = np.abs(U[0] - Ux).max() / scale
            assert e < max(3 * e_oracle, 1e-9), (variant, small, e, e_oracle)  # was 1.7e-7 (AM_DIV) / 2.2e-7 (EU)
            if lx is not None:
                el = np.abs(lam[0] - lx).max() / max(1.0, np.abs(lx).max())
                assert el < max(10 * np.abs(lo - lx).max() / max(1.0, np.abs(lx).max()), 1e-8), (small, el)  # was 1.8e-6


def test_rendezvous_timeout_sets_the_error_word(emu):
    """The pair rendezvous of the two-wavefront rows polls a bounded number of times.  A partner that never publishes
    (test hook: the high half withholds its token on v-row 1) must leave a code in the handle's error word -- the library
    turns it into HADI_ERR_INTERNAL -- and the kernel must still drain."""
    m1, m2, N = 600, 12, 1
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, [100.0])
    par = np.array([[Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]])
    dd = [np.array(x, dtype=np.float64) for x in Cm.DIVS]

    def run():
        U, lam = U0.copy(), np.zeros_like(U0)
        rc = emu.emu_solve(1, m1, m2, N, C.c_double(Cm.T / 10), C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(0.0), _P(par),
                           O.EU, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), 1, len(dd[0]), _P(dd[0]), _P(dd[1]),
                           _P(dd[2]), 64, 0, 0, None, None, None)
        assert rc == 0
        return emu.emu_take_error()

    emu.emu_set_tuning(b"strip", 1)  # paired strips (the shared ring's exchange is a block barrier under the emulator)
    try:
        assert run() == 0
        emu.emu_set_tuning(b"debug_fault", 1)
        assert run() == 1  # HADI_DEVERR_RENDEZVOUS
        emu.emu_set_tuning(b"debug_fault", 0)
        assert run() == 0  # the word is sticky until read, not beyond
    finally:
        emu.emu_set_tuning(b"reset", 0)


def test_instance_resident_team_kernel(emu):
    """hadi_team_kernel: the whole time loop of up to 8 European instances in one launch (row phase: hadi_strip_step on rows
    loaded straight to registers; column phase: hadi_pb_* on the team's blocks; team barriers in between).  Under the
    emulator a team is ONE block (blocks run one after the other), which still exercises every index of the two phases: 8 and 4
    nodes per lane, 1 / 2 / 4 / 8 column chunks, more and fewer rows than team wavefronts, two instances, r_f != 0, put data."""
    _run(emu, 300, 40, 2, [100.0, 93.0], O.EU, 8, small=4)           # 8 nodes per lane, 2 chunks
    _run(emu, 200, 100, 1, [100.0], O.EU, 8, r_f=0.01, small=4)      # 4 nodes per lane, 4 chunks
    _run(emu, 260, 20, 2, [100.0], O.EU, 8, small=4, put=True)       # one chunk: no exchange barrier
    _run(emu, 200, 40, 6, [100.0, 95.0], O.DIV, 8, small=4)          # discrete dividends: the jump inside the time loop (4 nodes per lane)
    _run(emu, 300, 20, 12, [100.0], O.DIV, 8, small=4, put=True)     # ... 8 nodes per lane, put data (ex-dividend spot <= 0 takes the s = 0 value)
    _run(emu, 512, 256, 1, [100.0], O.EU, 8, small=4)                # the benchmarked shape: 257 rows, 8 chunks, 9 column tiles
    # Teams of SEVERAL blocks (round 4: the emulator can run all blocks of a grid at once): formation counters, the team barrier
    # with its arrival counter, rows and column tiles split over the blocks, the rows other blocks wrote read back through
    # global memory.  2, 4 and 32 blocks per team (the last one the product's geometry: 256 wavefronts for 257 rows).
    for nb, cases in ((2, [(300, 40, 2, [100.0, 93.0], O.EU, {}), (200, 100, 3, [100.0], O.DIV, dict(r_f=0.01))]),
                      (4, [(512, 70, 2, [100.0, 96.0, 104.0], O.EU, dict(r_f=0.01)), (260, 130, 6, [100.0], O.DIV, dict(put=True))]),
                      (32, [(512, 256, 2, [100.0], O.EU, {})])):
        emu.emu_set_tuning(b"team_blocks", nb)
        try:
            for m1, m2, N, ks, var, kw in cases:
                _run(emu, m1, m2, N, ks, var, 8, small=4, **kw)
        finally:
            emu.emu_set_tuning(b"reset", 0)


def test_sequential_passes_for_shapes_beyond_the_streaming_kernels(emu):
    """m1 > 1024 (hadi_pass_a_seq: lane <-> v-row, rows in natural order) and m2 > 527 (hadi_pass_b_seq: lane <-> column,
    unchunked factorisation) -- the reference bounds a grid by its total size only.  Each alone with the streaming kernel of
    the other direction, both together, American and dividend variants, put data, r_f != 0, m1 a multiple of 64."""
    _run(emu, 1100, 12, 2, [100.0], O.EU, 8, r_f=0.01)        # sequential row pass + chunked column pass
    _run(emu, 1088, 40, 2, [100.0], O.AM, 8)                  # m1 = 17 * 64: the i = 0 slot sits right behind node m1
    _run(emu, 20, 528, 1, [100.0], O.EU, 8)                   # ring row pass + sequential column pass
    _run(emu, 70, 530, 1, [104.0], O.AM, 8)                   # 2 nodes per lane + sequential column pass, American
    _run(emu, 1030, 530, 1, [100.0], O.AM, 8, r_f=0.02)       # both sequential
    # (dividends and put data on the natural layout: tests/test_gpu_regressions.py::test_grids_beyond_1024_s_intervals_or_527_v_intervals)


def test_pair_strips_two_strips_per_wavefront(emu):
    """128 < m1 <= 256 on strips: hadi_pass_a_pairs runs the 8-nodes-per-lane arithmetic on two strips at once (lanes 0..31
    / 32..63), rows interleaved in the ring, row scalars per lane, five-level cyclic reduction inside each half.  Strips of
    equal and unequal length, an empty second strip, ascending and descending wavefronts, full width m1 = 256 and a short
    grid, r_f != 0 (the b1 node moves along the anti-diagonal through both halves), dividends, put data, American sweeps on
    the explicit pair and in the P representation, the row that carries b2 in either half."""
    emu.emu_set_tuning(b"strip", 1)
    try:
        _run(emu, 256, 54, 2, [100.0], O.EU, 1, r_f=0.01)              # 55 rows: 8 strips of 7 (the last: 6)
        _run(emu, 200, 40, 3, [100.0], O.EU, 1)                        # 41 rows: strips of 6, the eighth has 5... and r < m1 everywhere
        _run(emu, 130, 20, 2, [104.0], O.DIV, 1, put=True)             # 21 rows: 3 per strip, the last strip empty
        _run(emu, 256, 54, 2, [100.0], O.AM, 1)                        # explicit (U, lambda_bar) pair
        _run(emu, 256, 64, 2, [100.0], O.AM, 1, scheme=3)              # the P representation (4-slot ring, raw row re-read)
        _run(emu, 180, 33, 3, [100.0], O.AM_DIV, 1, scheme=3, r_f=0.02)
        emu.emu_set_tuning(b"strip_blocks", 2)                         # 16 strips per instance
        _run(emu, 200, 40, 2, [100.0], O.EU, 1)
    finally:
        emu.emu_set_tuning(b"reset", 0)


def _random_case(rng):
    """One random problem for the emulator sweep below: shape class, variant, scheme and the kernel-selection overrides the
    library's own tuning keys offer (the generator of tools/fuzz_parity.py is frozen; this one is the emulator's own)."""
    cls = rng.choice(["one", "two", "four", "eight", "wide", "seq_row", "seq_col", "tall", "lds", "team"])
    if cls == "lds":   # LDS-resident kernels: 4 or 8 wavefronts per instance, one wavefront per instance (pair of instances)
        variant = rng.choice([O.EU, O.AM, O.DIV, O.AM_DIV])
        small = rng.choice([1, 2]) if variant in (O.AM, O.AM_DIV) else rng.choice([1, 2, 3, 5])
        n = rng.choice([1, 2, 3])
        return dict(m1=rng.randint(8, 128), m2=rng.randint(4, 31), N=rng.randint(1, 3) if variant in (O.EU, O.AM) else rng.randint(4, 7),
                    strikes=[rng.uniform(85, 115) for _ in range(n)], variant=variant, scheme=0, put=rng.random() < 0.3,
                    r_f=rng.choice([0.0, 0.01, 0.03]), target_waves=8, tuning={}, small=small)
    if cls == "team":  # instance-resident launch: teams of 1, 2 or 4 blocks (all blocks of the grid at once)
        variant = rng.choice([O.EU, O.DIV])
        n = rng.choice([1, 2, 3])
        return dict(m1=rng.randint(129, 512), m2=rng.choice([rng.randint(8, 60), rng.randint(61, 263)]), N=rng.randint(1, 3) if variant == O.EU else rng.randint(4, 7),
                    strikes=[rng.uniform(85, 115) for _ in range(n)], variant=variant, scheme=0, put=rng.random() < 0.3,
                    r_f=rng.choice([0.0, 0.01, 0.03]), target_waves=8, tuning={"team_blocks": rng.choice([1, 2, 4])}, small=4)
    m1 = {"one": rng.randint(8, 64), "two": rng.randint(65, 128), "four": rng.randint(129, 256), "eight": rng.randint(257, 512),
          "wide": rng.randint(513, 1024), "seq_row": rng.randint(1025, 1100), "seq_col": rng.randint(20, 200),
          "tall": rng.randint(20, 140)}[cls]
    m2 = {"seq_col": rng.randint(528, 540), "tall": rng.randint(264, 520)}.get(cls, rng.randint(6, 70) if rng.random() < 0.8 else rng.randint(71, 200))
    seq = cls in ("seq_row", "seq_col")
    variant = rng.choice([O.EU, O.AM, O.DIV, O.AM_DIV])
    scheme = 0
    if not seq:
        if variant == O.EU and rng.random() < 0.3: scheme = 1
        elif variant == O.EU and rng.random() < 0.4: scheme = 2   # (the emulator driver has no widen / jump / narrow path for dividends)
        elif variant in (O.AM, O.AM_DIV) and rng.random() < 0.6: scheme = 3
    put = scheme in (0, 3) and rng.random() < 0.3
    tuning = {}
    if not seq and rng.random() < 0.6: tuning["strip"] = 1
    if cls == "four" and rng.random() < 0.5: tuning["pair_strips"] = 1
    if rng.random() < 0.2: tuning["strip_blocks"] = rng.choice([2, 3])
    if scheme == 1 and rng.random() < 0.3: tuning["cs_strips"] = 0
    if rng.random() < 0.2: tuning["col_prefetch"] = 1
    if rng.random() < 0.2: tuning["tile_interleave"] = 1
    n = rng.choice([1, 1, 2, 3])
    N = rng.randint(1, 3) if variant in (O.EU, O.AM) else rng.randint(4, 7)   # (the dividends land on steps 2 .. 6)
    return dict(m1=m1, m2=m2, N=N, strikes=[rng.uniform(85, 115) for _ in range(n)], variant=variant, scheme=scheme, put=put,
                r_f=rng.choice([0.0, 0.01, 0.03]), target_waves=rng.choice([1, 8]), tuning=tuning, small=0)


@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_and_kernel_choices_vs_oracle(emu, seed):
    """Since the emulator runs a wavefront's lanes as fibers (round 4) a sweep costs tenths of a second: 8 x 30 random problems
    -- every shape class (1 .. 8 nodes per lane, two wavefronts per row, the sequential passes beyond 1024 / 527 intervals,
    9 .. 16 column chunks, the LDS-resident kernels, the instance-resident launch with teams of 1 / 2 / 4 blocks), the four variants, Craig-Sneyd, the fp32 state, the P representation, put data, forced strips /
    pair strips / several blocks per instance / column-pass alternatives -- each against the oracle's full field."""
    import random
    rng = random.Random(1000 + seed)
    for k in range(25):
        c = _random_case(rng)
        # well-conditioned s-grids only: S_0 inserted a few 1e-6 beside a node leaves neighbouring intervals 1e5 apart and
        # cond * eps of round-off in BOTH fp64 solvers -- the GPU campaign sends such instances to the binary128 adjudicator
        # (DESIGN.md section 2); here the strikes are drawn again
        for _ in range(50):
            d = np.diff(Cm.oracle_grids(c["m1"], 8, c["strikes"])[0], axis=1)
            if np.maximum(d[:, 1:] / d[:, :-1], d[:, :-1] / d[:, 1:]).max() <= 30.0:
                break
            c["strikes"] = [rng.uniform(85, 115) for _ in c["strikes"]]
        for key, val in c["tuning"].items():
            assert emu.emu_set_tuning(key.encode(), val) == 0
        try:
            _run(emu, c["m1"], c["m2"], c["N"], c["strikes"], c["variant"], c["target_waves"], r_f=c["r_f"], scheme=c["scheme"], put=c["put"],
                 small=c["small"], tol=1e-10)  # (the bound of the GPU parity tests)
        except AssertionError as e:
            raise AssertionError("seed %d case %d: %r" % (seed, k, c)) from e
        finally:
            emu.emu_set_tuning(b"reset", 0)


# ---- the predictor-corrector schemes (Craig-Sneyd, Modified Craig-Sneyd, Hundsdorfer-Verwer) and per-instance step grids ----
# emu_solve's scheme codes: 0 Douglas, 1 CS, 3 Douglas with the American P representation, 4 MCS, 5 HV
EMU_CS, EMU_AMP, EMU_MCS, EMU_HV = 1, 3, 4, 5
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + np.sqrt(3.0) / 6.0
# per-instance model parameters (rho, sigma, kappa, eta) of the mixed batches below
PARS3 = [(-0.9, 0.3, 1.5, 0.04), (-0.5, 0.5, 2.0, 0.09), (0.3, 0.2, 0.5, 0.02)]


def _plan(emu, m1, m2, n, target_waves):
    """(B, G, use_strip, use_pairs) of the plan emu_solve starts from (the current tuning overrides applied)."""
    o = (C.c_longlong * 26)()
    assert emu.emu_plan_full(m1, m2, n, target_waves, o) == 0
    return int(o[0]), int(o[1]), bool(o[14]), bool(o[24])


def _run_pc(emu, m1, m2, strikes, scheme, target_waves, theta=Cm.THETA, r_f=0.0, N=2, Ns=None, dts=None, pars=None,
            variant=O.EU, tol=1e-10):
    """One batch through emu_solve, each instance's full field against its own reference solve: oracle.solve for Douglas / CS /
    the P representation, scheme_ref.solve_one for MCS / HV (built from the instance's own make_params).  Ns / dts: per-instance
    step counts and step sizes (emu_solve's N_i / dt_i; None: N steps of T / N for everybody).  pars: per-instance (rho, sigma,
    kappa, eta).  tol: relative to max |U_ref| of the instance (the bound of the GPU parity tests)."""
    import scheme_ref as S
    n = len(strikes)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes)
    pars = pars or [(Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)] * n
    par = np.ascontiguousarray(np.array(pars[:n], dtype=np.float64))
    Ni = np.array(Ns if Ns is not None else [N] * n, dtype=np.int32)
    dti = np.array(dts if dts is not None else [Cm.T / N] * n, dtype=np.float64)
    U, lam = U0.copy(), np.zeros_like(U0)
    dd = [np.array(x, dtype=np.float64) for x in Cm.DIVS]
    rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(theta), C.c_double(Cm.R_D), C.c_double(r_f), _P(par),
                       variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), target_waves, len(dd[0]), _P(dd[0]),
                       _P(dd[1]), _P(dd[2]), 64, 0, scheme, None,
                       Ni.ctypes.data_as(C.POINTER(C.c_int)) if Ns is not None else None, _P(dti) if Ns is not None else None)
    assert rc == 0, rc
    for k in range(n):
        p = O.make_params(m1, m2, int(Ni[k]), float(dti[k]), theta, Cm.R_D, r_f, *pars[k], variant,
                          scheme=1 if scheme == EMU_CS else 0)
        if scheme in (EMU_MCS, EMU_HV):
            Uo, lo = S.solve_one(p, vs[k], vv[k], ds[k], dv[k], U0[k], S.MCS if scheme == EMU_MCS else S.HV), None
        else:
            Uo, lo, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k], U0[k])
        scale = np.abs(Uo).max()
        err = np.abs(U[k] - Uo).max()
        assert err <= tol * scale, (k, err / scale)
        if variant in (O.AM, O.AM_DIV):
            assert np.abs(lam[k] - lo).max() <= 1e-9 * max(1.0, np.abs(lo).max()), k


@pytest.mark.parametrize("scheme,theta", [(EMU_MCS, TH_MCS), (EMU_HV, TH_HV)], ids=["MCS", "HV"])
def test_mcs_and_hv_on_ring_and_strips(emu, scheme, theta):
    """hadi_pass_a_strip_sch (predictor and corrector at 2, 4 and 8 nodes per lane; the corrector on paired strips, whose
    predictor runs on the shared ring) and hadi_pass_a_sch (`cs_strips` = 0, and the one-node-per-lane ring) against the
    restatement: the shapes of test_craig_sneyd_on_barrier_free_strips -- a short last strip, a strip without a partner, r_f != 0."""
    emu.emu_set_tuning(b"strip", 1)
    try:
        for m1, m2, N, ks, r_f, want in ((100, 20, 3, [100.0, 92.0], 0.01, (2, 1)), (200, 26, 2, [100.0], 0.0, (4, 1)),
                                         (300, 34, 2, [104.0], 0.02, (8, 1)), (700, 20, 2, [100.0], 0.01, (8, 2))):
            assert _plan(emu, m1, m2, len(ks), 1) == want + (True, False)
            for cs_strips in (1, 0):
                emu.emu_set_tuning(b"cs_strips", cs_strips)
                _run_pc(emu, m1, m2, ks, scheme, 1, theta=theta, r_f=r_f, N=N)
    finally:
        emu.emu_set_tuning(b"reset", 0)
    _run_pc(emu, 40, 12, [100.0, 91.0], scheme, 8, theta=theta, r_f=0.01, N=3)  # one node per lane


@pytest.mark.parametrize("scheme,theta", [(EMU_CS, 0.5), (EMU_MCS, TH_MCS), (EMU_HV, TH_HV)], ids=["CS", "MCS", "HV"])
def test_predictor_and_corrector_split_between_strips_and_ring(emu, scheme, theta):
    """`cs_strips` = 2 (only the predictor on strips, the corrector on the shared ring) and 3 (the other way round): the strip
    and ring kernels hand each other the R1 / C2 carry-over rows, so each must read what the other wrote."""
    emu.emu_set_tuning(b"strip", 1)
    try:
        for m1, m2, N, ks, r_f in ((100, 20, 2, [100.0, 92.0], 0.01), (200, 26, 2, [100.0], 0.0), (300, 34, 2, [104.0], 0.02)):
            for cs_strips in (2, 3):
                emu.emu_set_tuning(b"cs_strips", cs_strips)
                _run_pc(emu, m1, m2, ks, scheme, 1, theta=theta, r_f=r_f, N=N)
    finally:
        emu.emu_set_tuning(b"reset", 0)


MIXED = dict(Ns=[3, 1, 2], dts=[1.0 / 3.0, 0.45, 0.35], pars=PARS3)


@pytest.mark.parametrize("path,m1,m2,tuning,want", [
    ("ring", 40, 12, {}, (1, 1, False, False)),
    ("strips4", 200, 26, {"strip": 1}, (4, 1, True, False)),
    ("strips8", 300, 34, {"strip": 1}, (8, 1, True, False)),
    ("paired", 700, 20, {"strip": 1}, (8, 2, True, False)),
    ("pairs", 256, 54, {"strip": 1, "pair_strips": 1}, (4, 1, True, True)),
])
def test_mixed_maturities_and_per_instance_parameters(emu, path, m1, m2, tuning, want):
    """Multi-maturity batches (N_i = 3, 1, 2 with their own delta_t_i) with per-instance rho / sigma / kappa / eta on every row
    kernel: each kernel must take dt, theta dt, e_n / e_{n-1} and the MCS / HV constants from ITS instance's parameter block and
    leave the instances that have taken their last step alone (emu_solve poisons their Y / R1 / C2 and returns 5 if a row pass
    wrote there).  Douglas (European, American in the P representation), CS, MCS, HV; on `pairs` (hadi_pass_a_pairs) the
    predictor-corrector schemes run on the shared ring."""
    for k, v in tuning.items():
        emu.emu_set_tuning(k.encode(), v)
    try:
        ks, tw = [100.0, 93.0, 106.0], 1 if tuning else 8
        assert _plan(emu, m1, m2, 3, tw) == want
        _run_pc(emu, m1, m2, ks, 0, tw, r_f=0.01, **MIXED)
        _run_pc(emu, m1, m2, ks, EMU_AMP, tw, variant=O.AM, **MIXED)
        _run_pc(emu, m1, m2, ks, EMU_CS, tw, theta=0.5, r_f=0.01, **MIXED)
        _run_pc(emu, m1, m2, ks, EMU_MCS, tw, theta=TH_MCS, r_f=0.01, **MIXED)
        _run_pc(emu, m1, m2, ks, EMU_HV, tw, theta=TH_HV, r_f=0.01, **MIXED)
    finally:
        emu.emu_set_tuning(b"reset", 0)


def test_per_instance_step_grids_are_refused_with_dividends(emu):
    m1, m2 = 40, 12
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, [100.0])
    par = np.array([[Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]])
    dd = [np.array(x, dtype=np.float64) for x in Cm.DIVS]
    Ni, dti = np.array([4], dtype=np.int32), np.array([0.25])
    U = U0.copy()
    rc = emu.emu_solve(1, m1, m2, 4, C.c_double(0.25), C.c_double(Cm.THETA), C.c_double(Cm.R_D), C.c_double(0.0), _P(par),
                       O.DIV, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), None, 8, len(dd[0]), _P(dd[0]), _P(dd[1]),
                       _P(dd[2]), 64, 0, 0, None, Ni.ctypes.data_as(C.POINTER(C.c_int)), _P(dti))
    assert rc == 3


def _random_pc_case(rng):
    """One random predictor-corrector problem (the emulator's own generator, independent of _random_case and its seeds)."""
    scheme = rng.choice([EMU_CS, EMU_MCS, EMU_HV])
    theta = rng.choice({EMU_CS: [0.0, 0.3, 0.5, 1.0], EMU_MCS: [0.25, TH_MCS, 0.5, 0.75, 1.0],
                        EMU_HV: [0.5, 0.6, TH_HV, 1.0]}[scheme])
    cls = rng.choice(["one", "two", "four", "eight", "wide", "tall"])
    m1 = {"one": rng.randint(8, 64), "two": rng.randint(65, 128), "four": rng.randint(129, 256), "eight": rng.randint(257, 512),
          "wide": rng.randint(513, 1024), "tall": rng.randint(20, 140)}[cls]
    if cls == "tall":
        m2 = rng.randint(264, 527)
    elif rng.random() < 0.2:
        m2 = rng.randint(3, 5)
    else:
        m2 = rng.randint(6, 70)
    n = rng.choice([1, 2, 3])
    if rng.random() < 0.5:
        pars = [(rng.uniform(-0.9, 0.5), rng.uniform(0.1, 0.6), rng.uniform(0.5, 3.0), rng.uniform(0.02, 0.1)) for _ in range(n)]
    else:
        pars = None
    if rng.random() < 0.5:
        Ns = [rng.randint(1, 3) for _ in range(n)]
        dts = [rng.uniform(0.25, 1.5) / k for k in Ns]
    else:
        Ns = dts = None
    tuning = {}
    if rng.random() < 0.6: tuning["strip"] = 1
    if rng.random() < 0.6: tuning["cs_strips"] = rng.choice([0, 1, 2, 3])
    if cls == "four" and rng.random() < 0.5: tuning["pair_strips"] = 1
    if rng.random() < 0.2: tuning["strip_blocks"] = rng.choice([2, 3])
    if rng.random() < 0.25: tuning["col_prefetch"] = 1
    if rng.random() < 0.25: tuning["tile_interleave"] = 1
    N = rng.randint(1, 3)
    if theta == 0.0:  # explicit Craig-Sneyd: one step (more steps of these sizes grow without bound, round-off with them)
        N, Ns = 1, Ns and [1] * n
    return dict(m1=m1, m2=m2, N=N, strikes=[rng.uniform(85, 115) for _ in range(n)], scheme=scheme, theta=theta,
                r_f=rng.choice([0.0, 0.01, 0.03, Cm.R_D, 0.06]), target_waves=rng.choice([1, 8]), tuning=tuning, pars=pars,
                Ns=Ns, dts=dts)


@pytest.mark.parametrize("seed", range(8))
def test_random_predictor_corrector_cases_vs_references(emu, seed):
    """8 x 20 random CS / MCS / HV problems: theta off the usual values (MCS above 1/2 and at 1, HV at and above 1/2, CS at 0
    and 1), r_f = 0, r_f = r_d (the library then keeps the strips off) and r_f > r_d, every streaming shape class incl. 9 .. 16
    column chunks and grids of 4 .. 6 v-nodes, per-instance parameters and maturities, `cs_strips` 0 .. 3, strip / pair-strip /
    strip-block / column-pass overrides -- each instance's full field against its own reference solve."""
    import random
    rng = random.Random(7000 + seed)
    for k in range(20):
        c = _random_pc_case(rng)
        for _ in range(50):  # well-conditioned s-grids only (see test_random_shapes_and_kernel_choices_vs_oracle)
            d = np.diff(Cm.oracle_grids(c["m1"], 8, c["strikes"])[0], axis=1)
            if np.maximum(d[:, 1:] / d[:, :-1], d[:, :-1] / d[:, 1:]).max() <= 30.0:
                break
            c["strikes"] = [rng.uniform(85, 115) for _ in c["strikes"]]
        for key, val in c["tuning"].items():
            assert emu.emu_set_tuning(key.encode(), val) == 0
        try:
            _run_pc(emu, c["m1"], c["m2"], c["strikes"], c["scheme"], c["target_waves"], theta=c["theta"], r_f=c["r_f"], N=c["N"],
                    Ns=c["Ns"], dts=c["dts"], pars=c["pars"])
        except AssertionError as e:
            raise AssertionError("seed %d case %d: %r" % (seed, k, c)) from e
        finally:
            emu.emu_set_tuning(b"reset", 0)


def test_graph_key_lists_every_pointer_of_the_sweep_arguments(emu):
    """A captured time loop bakes the whole HadiSweepArgs block into its nodes, so the graph key (run_sweep) takes every address
    in it from hadi_sweep_args_ptrs.  Each pointer-sized word of the struct outside L and the int fields -- rs_tab, the
    paired strips' coupling table, among them -- must change that list when it changes; a pointer the helper forgets would let
    a call replay a graph whose nodes hold another buffer's address."""
    out = (C.c_int * 32)()
    words = C.c_int()
    bad = emu.emu_sweep_args_unkeyed(out, 32, C.byref(words))
    assert words.value == 15, words.value  # U Y LAM R1 C2 rs_tab U0 pay_mis scoef b2row rowc pb rinv ipar err
    assert bad == 0, "pointer words missing from the graph key at byte offsets %s" % list(out[:min(bad, 32)])
