"""CPU-only: every kernel family of the wave emulator on batches whose instances carry DIFFERENT v-grids
(Cm.mixed_vgrid_batch: V, V_0 and d move from instance to instance, so rowc / pb / rinv / a2i / b2row, the paired strips'
coupling table, the team kernel's RT, the resident sweep's staged invariants and the tables of the two-instances-per-wavefront
kernel all differ between neighbours).  A kernel that read instance 0's, a neighbour's or a sub-batch's first v-derived table
would be off by 1e-3 .. 1e-2 of max|U| here (test_a_wrong_instances_v_grid_cannot_pass); the bound is the one of
test_emu_kernel_logic.py.  One case per family, at the shape, target_waves, `small` and tuning that family's own test uses."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import scheme_ref as S
import test_emu_resident as ER
import test_emu_small_sch as ES
from test_emu_kernel_logic import EMU_CS, EMU_HV, EMU_MCS, TH_HV, TH_MCS, _P, _plan, emu  # noqa: F401  (emu: the module's fixture)
from test_emu_resident import emu as emu_resident  # noqa: F401
from test_emu_small_sch import emu as emu_small_sch  # noqa: F401

EMU_F32, EMU_AMP = 2, 3
TOL = 1e-11  # of max|U_ref| of the instance (test_emu_kernel_logic._run); the fp32 state: 2e-7 N


def _batch(m1, m2, n, put=False, same_v0=None):
    strikes, g, v0s = Cm.mixed_vgrid_batch(m1, m2, n, same_v0)
    U0 = g.put_payoff(strikes) if put else g.call_payoff(strikes)
    return strikes, g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, U0


def test_helper_batches_are_mixed_and_well_conditioned():
    """At least four distinct candidates obey the 30x rule at every m2 the mixed tests use (the helper asserts it), the row of
    V_0 moves with the candidate, and the common-V_0 list keeps V_0 a node of every grid."""
    for m2 in (12, 20, 25, 26, 30, 32, 34, 40, 50, 54, 60, 64, 70, 80, 100, 128, 140, 150, 256, 263, 264, 265, 270, 300, 528, 600):
        for kw in ({}, {"vary_vd": False}, {"same_v0": Cm.V_0_ALT}):
            cand = Cm.mixed_vgrid_candidates(m2, **kw)
            assert len(set(cand)) == len(cand) >= Cm.MIXED_MIN, (m2, kw, cand)
    for same in (None, Cm.V_0_ALT):
        strikes, g, v0s = Cm.mixed_vgrid_batch(50, 25, 6, same)
        rows = [O.find_v_index(g.Vec_v[k], v0s[k]) for k in range(6)]
        assert all(g.Vec_v[k][r] == v0s[k] for k, r in enumerate(rows)) and len(set(rows)) >= 3, rows
        assert all(not np.array_equal(g.Vec_v[k], g.Vec_v[k + 1]) for k in range(5))
        assert same is None or set(v0s) == {same}


def test_a_wrong_instances_v_grid_cannot_pass():
    """The oracle field of instance 1 on its own v-grid and on instance 0's differ by far more than any bound in use: a read of
    the wrong instance's v-derived table is not a rounding-level event."""
    m1, m2, N = 50, 25, 2
    strikes, vs, vv, ds, dv, U0 = _batch(m1, m2, 3)
    p = Cm.oracle_params(m1, m2, N, "EU")
    own, _, _ = O.solve(p, vs[1], vv[1], ds[1], dv[1], U0[1])
    for other in (0, 2):
        wrong, _, _ = O.solve(p, vs[1], vv[other], ds[1], dv[other], U0[1])
        diff = np.abs(own - wrong).max() / np.abs(own).max()
        print("instance 1 on the v-grid of instance %d: %.2e of max|U|" % (other, diff))
        assert diff > 1e-6


def _run(emu, m1, m2, N, n, variant, target_waves, r_f=0.0, small=0, scheme=0, put=False, theta=Cm.THETA, tol=TOL):
    """test_emu_kernel_logic._run on a mixed-v-grid batch: every instance against the reference solved on ITS grids (oracle;
    scheme_ref for MCS / HV), full field and lambda_bar."""
    strikes, vs, vv, ds, dv, U0 = _batch(m1, m2, n, put)
    ks = np.array(strikes, dtype=np.float64)
    divs = Cm.DIVS
    U, lam = U0.copy(), np.zeros_like(U0)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (n, 1)).copy()
    dd = [np.array(x, dtype=np.float64) for x in divs]
    rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(theta), C.c_double(Cm.R_D), C.c_double(r_f), _P(par),
                       variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), target_waves, len(dd[0]), _P(dd[0]),
                       _P(dd[1]), _P(dd[2]), 64, small, scheme, _P(ks) if put else None, None, None)
    assert rc == 0, rc
    worst = 0.0
    for k in range(n):
        p = O.make_params(m1, m2, N, Cm.T / N, theta, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, variant,
                          divs if variant in (O.DIV, O.AM_DIV) else None, option_type=O.PUT if put else O.CALL,
                          strikes=ks[k:k + 1] if put else None)
        p.scheme = 1 if scheme == EMU_CS else 0
        p.state_fp32 = 1 if scheme == EMU_F32 else 0
        if scheme in (EMU_MCS, EMU_HV):
            Uo, lo = S.solve_one(p, vs[k], vv[k], ds[k], dv[k], U0[k], S.MCS if scheme == EMU_MCS else S.HV), None
        else:
            Uo, lo, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k], U0[k])
        assert np.isfinite(Uo).all()
        err = np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        worst = max(worst, err)
        assert err < (2e-7 * N if scheme == EMU_F32 else tol), (k, err)
        if lo is not None:
            assert np.abs(lam[k] - lo).max() < 1e-9 * max(1.0, np.abs(lo).max()), k
    print("%dx%d n=%d variant %d scheme %d small %d: worst field error %.2e" % (m1, m2, n, variant, scheme, small, worst))


def _tuned(emu, tuning, m1, m2, N, n, variant, tw, want=None, **kw):
    """want: (B, G, use_strip, use_pairs) the plan must give under this tuning -- the family the case is named after."""
    for k, v in tuning.items():
        assert emu.emu_set_tuning(k.encode(), v) == 0
    try:
        assert want is None or _plan(emu, m1, m2, n, tw) == want, (_plan(emu, m1, m2, n, tw), want)
        _run(emu, m1, m2, N, n, variant, tw, **kw)
    finally:
        emu.emu_set_tuning(b"reset", 0)


#        id                     tuning                                   m1   m2   N  n  variant   tw  keywords
CASES = [("ring_one_node",      {},                                      40,  12,  3, 4, O.EU,     8,  dict(r_f=0.01)),
         ("ring_two_nodes",     {},                                      100, 20,  2, 3, O.EU,     8,  {}),
         ("strips",             {"strip": 1},                            300, 150, 1, 3, O.EU,     1,  dict(r_f=0.01)),
         ("strips_forced_am",   {"strip": 1},                            280, 40,  2, 3, O.AM,     1,  {}),
         ("pairs",              {"strip": 1, "pair_strips": 1},          256, 54,  2, 3, O.EU,     1,  dict(r_f=0.01)),
         ("paired_strips",      {"strip": 1},                            600, 26,  2, 3, O.EU,     1,  dict(r_f=0.01)),
         ("two_wave_ring",      {},                                      600, 12,  2, 3, O.EU,     8,  {}),
         ("col_chunked_div",    {},                                      72,  70,  6, 3, O.DIV,    3,  {}),
         ("col_9_chunks_am",    {},                                      70,  265, 1, 3, O.AM,     1,  dict(r_f=0.01)),
         ("col_b2_prefetch",    {"col_prefetch": 1, "tile_interleave": 1}, 100, 270, 1, 3, O.EU,   1,  {}),
         ("col_b1",             {"col_prefetch": 0, "tile_interleave": 0}, 100, 270, 1, 3, O.EU,   1,  {}),
         ("row_seq",            {},                                      1100, 12, 2, 3, O.EU,     8,  dict(r_f=0.01)),
         ("col_seq",            {},                                      20,  528, 1, 3, O.EU,     8,  {}),
         ("small_4_waves",      {},                                      50,  25,  6, 3, O.EU,     8,  dict(small=1)),
         ("small_4_waves_amdiv", {},                                     50,  25,  12, 3, O.AM_DIV, 8, dict(small=1)),
         ("small_8_waves",      {},                                      50,  25,  6, 3, O.AM_DIV, 8,  dict(small=2)),
         ("small_seq",          {},                                      50,  25,  3, 3, O.EU,     8,  dict(small=3)),
         ("small_seq2_odd_n",   {},                                      50,  25,  3, 5, O.EU,     8,  dict(small=5)),
         ("small_seq2_div_put", {},                                      40,  12,  12, 3, O.DIV,   8,  dict(small=5, r_f=0.01, put=True)),
         ("team_one_block",     {},                                      300, 40,  2, 3, O.EU,     8,  dict(small=4)),
         ("team_one_block_div", {},                                      200, 40,  6, 3, O.DIV,    8,  dict(small=4)),
         ("team_4_blocks",      {"team_blocks": 4},                      512, 70,  2, 3, O.EU,     8,  dict(small=4, r_f=0.01)),
         ("team_32_blocks",     {"team_blocks": 32},                     512, 256, 2, 2, O.EU,     8,  dict(small=4)),
         ("american_explicit",  {},                                      40,  12,  3, 3, O.AM,     4,  {}),
         ("american_p",         {},                                      40,  12,  4, 3, O.AM,     4,  dict(r_f=0.01, scheme=EMU_AMP)),
         ("american_p_strips",  {"strip": 1},                            300, 70,  2, 3, O.AM,     1,  dict(r_f=0.01, scheme=EMU_AMP)),
         ("dividends_strips",   {"strip": 1},                            200, 60,  10, 3, O.AM_DIV, 1, dict(r_f=0.01)),
         ("put_ring",           {},                                      40,  12,  3, 3, O.EU,     8,  dict(put=True)),
         ("put_strips_am",      {"strip": 1},                            300, 40,  2, 3, O.AM,     1,  dict(put=True)),
         ("fp32_ring",          {},                                      40,  12,  3, 3, O.EU,     8,  dict(r_f=0.01, scheme=EMU_F32)),
         ("fp32_strips",        {"strip": 1},                            300, 150, 1, 3, O.EU,     1,  dict(r_f=0.01, scheme=EMU_F32)),
         ("fp32_paired_strips", {"strip": 1},                            600, 26,  2, 3, O.EU,     1,  dict(scheme=EMU_F32))]


# (nodes per lane B, wavefronts per row G, strips, two strips per wavefront): the plan the row-pass families must run on
PLANS = {"ring_one_node": (1, 1, False, False), "ring_two_nodes": (2, 1, False, False), "strips": (8, 1, True, False),
         "strips_forced_am": (8, 1, True, False), "pairs": (4, 1, True, True), "paired_strips": (8, 2, True, False),
         "two_wave_ring": (8, 2, False, False), "american_p_strips": (8, 1, True, False), "dividends_strips": (4, 1, True, False),
         "put_strips_am": (8, 1, True, False), "fp32_strips": (8, 1, True, False), "fp32_paired_strips": (8, 2, True, False)}


@pytest.mark.parametrize("name,tuning,m1,m2,N,n,variant,tw,kw", CASES, ids=[c[0] for c in CASES])
def test_family_on_mixed_v_grids(emu, name, tuning, m1, m2, N, n, variant, tw, kw):
    _tuned(emu, tuning, m1, m2, N, n, variant, tw, want=PLANS.get(name), **kw)


@pytest.mark.parametrize("scheme,theta", [(EMU_CS, 0.5), (EMU_MCS, TH_MCS), (EMU_HV, TH_HV)], ids=["CS", "MCS", "HV"])
@pytest.mark.parametrize("path,tuning,m1,m2,N,tw,r_f", [("ring", {}, 40, 12, 3, 8, 0.01), ("strips", {"strip": 1}, 300, 34, 2, 1, 0.02),
                                                        ("paired_strips", {"strip": 1}, 700, 20, 2, 1, 0.01)],
                         ids=["ring", "strips", "paired_strips"])
def test_schemes_on_mixed_v_grids(emu, path, tuning, m1, m2, N, tw, r_f, scheme, theta):
    want = {"ring": (1, 1, False, False), "strips": (8, 1, True, False), "paired_strips": (8, 2, True, False)}[path]
    _tuned(emu, tuning, m1, m2, N, 3, O.EU, tw, want=want, r_f=r_f, scheme=scheme, theta=theta)


def test_resident_sweep_on_mixed_v_grids(emu_resident):
    """emu_solve_resident takes [n] v-grids: the invariants a block stages once are its own instance's."""
    m1, m2, N, n = 300, 80, 3, 3
    strikes, vs, vv, ds, dv, U0 = _batch(m1, m2, n)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (n, 1)).copy()
    ks = np.ascontiguousarray(strikes, dtype=np.float64)
    Ur, P = U0.copy(), C.c_int(0)
    rc = emu_resident.emu_solve_resident(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D),
                                         C.c_double(ER.R_F), _P(par), _P(vs), _P(vv), _P(ds), _P(dv), _P(Ur), 64, None, None,
                                         C.byref(P), _P(ks), 0)
    assert rc == 0 and P.value == 3, (rc, P.value)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, ER.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
    Uo, _, _ = O.solve_batch(p, vs, vv, ds, dv, U0)
    err = (np.abs(Ur - Uo).max(axis=1) / np.abs(Uo).max(axis=1)).max()
    print("resident sweep, mixed v-grids: worst field error %.2e" % err)
    assert err <= 1e-10  # (the bound of test_emu_resident._check)


@pytest.mark.parametrize("scheme,theta,name", ES.SCHEMES, ids=[s[2] for s in ES.SCHEMES])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_small_scheme_kernel_on_mixed_v_grids(emu_small_sch, m1, m2, scheme, theta, name):
    """emu_small_sch takes [n] v-grids: one and two nodes per lane, three instances with three v-grids."""
    n, N = 3, 2
    strikes, vs, vv, ds, dv, U0 = _batch(m1, m2, n)
    grids = (vs, vv, ds, dv, U0)
    U, _ = ES._emu_run(emu_small_sch, m1, m2, grids, scheme, theta, ES.R_F, [ES.MODEL] * n, [N] * n, [Cm.T / N] * n)
    worst = 0.0
    for k in range(n):
        Uo = ES._ref_one(m1, m2, grids, k, scheme, theta, ES.R_F, ES.MODEL, N, Cm.T / N)
        worst = max(worst, np.abs(U[k] - Uo).max() / np.abs(Uo).max())
    print("hadi_small_sch_kernel %s %dx%d, mixed v-grids: worst field error %.2e" % (name, m1, m2, worst))
    assert worst <= 1e-10  # (the bound of test_emu_small_sch._check)
