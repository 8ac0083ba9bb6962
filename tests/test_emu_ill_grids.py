"""CPU-only: every kernel family of the wave emulator on ILL-conditioned grids, the tiny interval placed on purpose
(tests/ill_grids.py: against lanes and wavefronts on the s-axis, against column chunks, strips and the last rows on the v-axis)
and judged by the frozen adjudication rule (ill_grids.judge: cap, band, else binary128 with the oracle's own distance over the
neighbourhood as the yardstick).  The twin of tests/test_gpu_ill_grids.py for kernel logic: a failure on the device can be
localised here without a GPU.

The family table is the one of tests/test_emu_mixed_vgrids.py (shape, target_waves, `small`, tuning and plan of each family), with
N = 3 -- the dividend variants keep the table's N: with fewer than five steps no dividend date meets the reference's dating rule
and the sweep would be a European one.  The fp32 state has its own yardstick and is not run here.  MCS and HV have no exact
reference (nothing under oracle/ knows them): finite and the sanity cap against tests/scheme_ref.py, the difference printed."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import ill_grids as I
import scheme_ref as S
import test_emu_mixed_vgrids as MV
import test_emu_resident as ER
import test_emu_small_sch as ES
from test_emu_kernel_logic import EMU_CS, EMU_HV, EMU_MCS, TH_HV, TH_MCS, _P, emu  # noqa: F401  (emu: the module's fixture)
from test_emu_resident import emu as emu_resident  # noqa: F401
from test_emu_small_sch import emu as emu_small_sch  # noqa: F401

AXES_TURNS = [("s", 0), ("s", 1), ("v", 0), ("v", 1)]
AT_IDS = ["%s%d" % at for at in AXES_TURNS]


def _plan(emu, m1, m2, n, tw):
    """(B, G, use_strip, use_pairs), strip height or None."""
    o = (C.c_longlong * 26)()
    assert emu.emu_plan_full(m1, m2, n, tw, o) == 0
    return (int(o[0]), int(o[1]), bool(o[14]), bool(o[24])), (int(o[15]) if o[14] else None)


def n_instances(m1, m2, axis, strip_rows=None):
    """One instance per position of the axis."""
    return len(I.s_positions(m1, 100.0)) if axis == "s" else len(I.v_positions(m2, strip_rows))


def _emu_solve(emu, insts, c, tw, small=0, scheme=0):
    ks, vs, vv, ds, dv, U0 = I.arrays(insts, c.put)
    n, m1, m2 = len(insts), insts[0].m1, insts[0].m2
    U, lam = U0.copy(), np.zeros_like(U0)
    par = np.tile(np.array(c.model), (n, 1)).copy()
    dd = [np.array(x, dtype=np.float64) for x in (c.divs or Cm.DIVS)]
    rc = emu.emu_solve(n, m1, m2, c.N, C.c_double(Cm.T / c.N), C.c_double(c.theta), C.c_double(Cm.R_D), C.c_double(c.r_f), _P(par),
                       c.variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), tw, len(dd[0]), _P(dd[0]), _P(dd[1]),
                       _P(dd[2]), 64, small, scheme, _P(ks) if c.put else None, None, None)
    assert rc == 0, rc
    return U, (lam if c.variant in (O.AM, O.AM_DIV) else None)


def _cap_only(name, c, insts, U, which):
    """MCS / HV: finite and the sanity cap against tests/scheme_ref.py; the difference is printed, nothing else is claimed."""
    ks, vs, vv, ds, dv, U0 = I.arrays(insts)
    worst = 0.0
    for k, inst in enumerate(insts):
        Uo = S.solve_one(I.params(c, inst), vs[k], vv[k], ds[k], dv[k], U0[k], which)
        assert np.isfinite(U[k]).all() and np.isfinite(Uo).all(), (name, k)
        d = np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        print("  %s #%d %s: |U - U_ref| %.2e of max|U_ref|" % (name, k, I.describe(inst), d))
        assert d <= I.CAP_U, (name, k, d)
        worst = max(worst, d)
    print("%s: worst %.2e (cap %.0e)" % (name, worst, I.CAP_U))


def _family(emu, name, tuning, m1, m2, N, variant, tw, axis, turn, want=None, r_f=0.0, small=0, scheme=0, put=False, theta=Cm.THETA):
    for k, v in tuning.items():
        assert emu.emu_set_tuning(k.encode(), v) == 0
    try:
        n = n_instances(m1, m2, axis)
        plan, rs = _plan(emu, m1, m2, n, tw)
        if axis == "v" and rs is not None and small == 0:
            n = n_instances(m1, m2, axis, rs)
            plan, rs2 = _plan(emu, m1, m2, n, tw)
            assert rs2 == rs, (rs, rs2)
        else:
            rs = None
        assert want is None or plan == want, (plan, want)
        c = I.cfg(N, theta=theta, r_f=r_f, variant=variant, scheme=1 if scheme == EMU_CS else 0, put=put)
        insts = I.admit(c, I.batch(m1, m2, n, axis, turn, rs))
        U, lam = _emu_solve(emu, insts, c, tw, small, scheme)
    finally:
        emu.emu_set_tuning(b"reset", 0)
    label = "%s %s turn %d" % (name, axis, turn)
    if scheme in (EMU_MCS, EMU_HV):
        _cap_only(label, c, insts, U, S.MCS if scheme == EMU_MCS else S.HV)
        return
    ok, verdicts = I.judge_batch(label, c, insts, U, lam)
    assert ok, [(k, v) for k, v in enumerate(verdicts) if not v["ok"]]
    return insts, verdicts


CASES = [c for c in MV.CASES if c[8].get("scheme") != MV.EMU_F32]


@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
@pytest.mark.parametrize("name,tuning,m1,m2,N,n,variant,tw,kw", CASES, ids=[c[0] for c in CASES])
def test_douglas_family(emu, name, tuning, m1, m2, N, n, variant, tw, kw, axis, turn):
    N = N if variant in (O.DIV, O.AM_DIV) else 3
    _family(emu, name, tuning, m1, m2, N, variant, tw, axis, turn, want=MV.PLANS.get(name), **kw)


@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
@pytest.mark.parametrize("scheme,theta", [(EMU_CS, 0.5), (EMU_MCS, TH_MCS), (EMU_HV, TH_HV)], ids=["CS", "MCS", "HV"])
@pytest.mark.parametrize("path,tuning,m1,m2,tw,r_f", [("ring", {}, 40, 12, 8, 0.01), ("strips", {"strip": 1}, 300, 34, 1, 0.02),
                                                      ("paired_strips", {"strip": 1}, 700, 20, 1, 0.01)],
                         ids=["ring", "strips", "paired_strips"])
def test_scheme(emu, path, tuning, m1, m2, tw, r_f, scheme, theta, axis, turn):
    """Craig-Sneyd by the rule (the adjudicator takes scheme = 1); MCS and HV on the same paths, finite and under the cap."""
    want = {"ring": (1, 1, False, False), "strips": (8, 1, True, False), "paired_strips": (8, 2, True, False)}[path]
    _family(emu, "%s %s" % ({EMU_CS: "CS", EMU_MCS: "MCS", EMU_HV: "HV"}[scheme], path), tuning, m1, m2, 3, O.EU, tw, axis, turn,
            want=want, r_f=r_f, scheme=scheme, theta=theta)


@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
@pytest.mark.parametrize("scheme,theta,name", ES.SCHEMES, ids=[s[2] for s in ES.SCHEMES])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_small_scheme_kernel(emu_small_sch, m1, m2, scheme, theta, name, axis, turn):
    """hadi_small_sch_kernel, one and two nodes per lane."""
    n, N = n_instances(m1, m2, axis), 3
    c = I.cfg(N, theta=theta, r_f=ES.R_F, scheme=1 if scheme == S.CS else 0, model=ES.MODEL)
    insts = I.admit(c, I.batch(m1, m2, n, axis, turn))
    ks, vs, vv, ds, dv, U0 = I.arrays(insts)
    U, _ = ES._emu_run(emu_small_sch, m1, m2, (vs, vv, ds, dv, U0), scheme, theta, ES.R_F, [ES.MODEL] * n, [N] * n, [Cm.T / N] * n)
    label = "hadi_small_sch_kernel %s %dx%d %s turn %d" % (name, m1, m2, axis, turn)
    if scheme != S.CS:
        _cap_only(label, c, insts, U, scheme)
        return
    ok, verdicts = I.judge_batch(label, c, insts, U)
    assert ok, [(k, v) for k, v in enumerate(verdicts) if not v["ok"]]


@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
def test_resident_sweep(emu_resident, axis, turn):
    """hadi_sweep_resident on 300x80 (three chunks, strips of 11 rows: small enough for the fibers), every position of the axis."""
    m1, m2, N = 300, 80, 3
    rs, _ = ER._strip_rows(m2)
    n = n_instances(m1, m2, axis, rs)
    c = I.cfg(N, r_f=ER.R_F)
    insts = I.admit(c, I.batch(m1, m2, n, axis, turn, rs if axis == "v" else None))
    ks, vs, vv, ds, dv, U0 = I.arrays(insts)
    par = np.tile(np.array([Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA]), (len(insts), 1)).copy()
    Ur, P = U0.copy(), C.c_int(0)
    rc = emu_resident.emu_solve_resident(len(insts), m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(Cm.R_D),
                                         C.c_double(ER.R_F), _P(par), _P(vs), _P(vv), _P(ds), _P(dv), _P(Ur), 64, None, None,
                                         C.byref(P), _P(ks), 0)
    assert rc == 0 and P.value == 3, (rc, P.value)
    ok, verdicts = I.judge_batch("resident sweep %s turn %d" % (axis, turn), c, insts, Ur)
    assert ok, [(k, v) for k, v in enumerate(verdicts) if not v["ok"]]


# ---- the device's reciprocal (twin of tests/test_gpu_regressions.py::test_two_wavefront_rows_with_a_tiny_interval_astride) ----
@pytest.fixture(scope="module")
def emu_device_rcp():
    """The emulator built with HADI_EMU_DEVICE_RCP: hadi_rcp rounds as on the device (a seed with the relative error of v_rcp_f64
    and the product's Newton steps) instead of by an IEEE division -- the one arithmetic difference between the two builds that
    an ill-conditioned grid amplifies."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    so = os.path.join(here, "emu", "libhadi_emu_devrcp.so")
    srcs = [os.path.join(here, "emu", f) for f in ("emu_driver.cpp", "wave_emu.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU", "-DHADI_EMU_DEVICE_RCP",
                               "-I" + os.path.join(here, "emu"), "-I" + csrc, "-o", so, os.path.join(here, "emu", "emu_driver.cpp")])
    lib = C.CDLL(so)
    lib.emu_set_tuning(b"reset", 0)
    return lib


@pytest.mark.parametrize("turn", [0, 1])
@pytest.mark.parametrize("what,variant,scheme,put", [("put", O.EU, 0, True), ("am_p", O.AM, MV.EMU_AMP, False), ("call", O.EU, 0, False)],
                         ids=["put", "am_p", "call"])
@pytest.mark.parametrize("path,tuning,tw,want", [("ring", {}, 8, (8, 2, False, False)), ("paired_strips", {"strip": 1}, 1, (8, 2, True, False))],
                         ids=["ring", "paired_strips"])
def test_two_wavefront_rows_with_the_devices_reciprocal(emu_device_rcp, path, tuning, tw, want, what, variant, scheme, put, turn):
    """600x40, the tiny interval astride the two wavefronts of a row among the positions.  With hadi_rcp's one Newton step in the
    cyclic reduction of such rows -- every reciprocal low by up to 2^-49 -- the pair's 2x2 determinant 1 - Bc Dd ~ 1 / R amplified
    the bias: under this build, before hadi_rcp_acc, 1.0e-7 of max|U| from binary128 on the last v-row where the oracle is 3.4e-9
    (put data, R = 1e6; on the device 1.45e-7, 43x the yardstick), 1.5e-8 against 6.3e-10 on the American sweep (R = 1e5), 5.3e-9
    against 1.1e-10 at R = 1e4 (30x, 23x and 25x the yardstick).  With the third-order step on those reciprocals: 7.9e-9, 1.7e-9
    and 8.0e-10."""
    insts, verdicts = _family(emu_device_rcp, "device reciprocal, %s %s" % (path, what), tuning, 600, 40, 3, variant, tw, "s", turn,
                              want=want, r_f=0.01, scheme=scheme, put=put)
    v = next(v for i, v in zip(insts, verdicts) if i.sname == "astride two wavefronts")
    # pinned as the adjudicated relation (before the fix: 30x, 23x and 25x the yardstick; after: at most 4.5x)
    assert v["stage"] == "band" or v["ratio"] < 10, v


def shapes_used():
    """Every (m1, m2, sweep) this file runs, for tests/test_oracle_ill_grids.py: (m1, m2, N, theta, r_f, variant, scheme, put)."""
    out = set()
    for name, tuning, m1, m2, N, n, variant, tw, kw in CASES:
        out.add((m1, m2, N if variant in (O.DIV, O.AM_DIV) else 3, Cm.THETA, kw.get("r_f", 0.0), variant, 0, kw.get("put", False)))
    for m1, m2, r_f in ((40, 12, 0.01), (300, 34, 0.02), (700, 20, 0.01)):
        out.add((m1, m2, 3, 0.5, r_f, O.EU, 1, False))
    for m1, m2 in ((50, 25), (100, 20)):
        out.add((m1, m2, 3, 0.5, ES.R_F, O.EU, 1, False))
    out.add((300, 80, 3, Cm.THETA, ER.R_F, O.EU, 0, False))
    return out
