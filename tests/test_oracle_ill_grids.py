"""CPU-only, no emulator: the conditions tests/test_emu_ill_grids.py and tests/test_gpu_ill_grids.py stand on.

On every (shape, sweep, axis, turn) those two files use: the construction assertions of tests/ill_grids.py hold (they are part of
building a batch), the fp64 oracle is finite, and its own distance from binary128 is at most 1e-4 / 31 in the field and 1e-3 / 31 in
lambda_bar -- so the reference alone can never trip the sanity cap while a solver is still within 30x of it -- and the yardstick is
deterministic.  The strip-edge position needs a plan and is placed by the two files themselves; its construction is covered here
by the scan over every raw interval.  ill_grids.judge is unit-tested on synthetic triples, one per outcome of the rule."""
import numpy as np
import pytest

import common as Cm
import ill_grids as I
import test_emu_ill_grids as EI
import test_gpu_ill_grids as GI

SWEEPS = sorted(EI.shapes_used() | GI.shapes_used())


def _id(s):
    m1, m2, N, theta, r_f, variant, scheme, put = s
    return "%dx%d-N%d-th%.2f-rf%g-v%d%s%s" % (m1, m2, N, theta, r_f, variant, "-CS" if scheme else "", "-put" if put else "")


@pytest.mark.parametrize("sweep", SWEEPS, ids=[_id(s) for s in SWEEPS])
def test_reference_distance_leaves_the_cap_alone(sweep):
    m1, m2, N, theta, r_f, variant, scheme, put = sweep
    c = I.cfg(N, theta=theta, r_f=r_f, variant=variant, scheme=scheme, put=put)
    insts = []
    for axis in ("s", "v"):
        n = len(I.s_positions(m1, 100.0)) if axis == "s" else len(I.v_positions(m2))
        for turn in (0, 1):
            insts += list(I.batch(m1, m2, n, axis, turn))
    before = insts
    insts = I.admit(c, tuple(insts))
    assert I.admit(c, insts) == insts  # (deterministic, and a fixed point)
    dist = [I.oracle_distance(c, i) for i in insts]
    dropped = [(I.describe(a), I.describe(b)) for a, b in zip(before, insts) if a != b]
    worst = max(d[0] for d in dist)
    worst_l = max((d[1] for d in dist if d[1] is not None), default=None)
    print("%s: %d instances, %d with a dropped ratio, oracle vs binary128: field %.2e%s" % (
        _id(sweep), len(insts), len(dropped), worst, "" if worst_l is None else ", lambda_bar %.2e" % worst_l))
    for inst, (eU, eL) in zip(insts, dist):
        assert np.isfinite(eU) and eU <= I.CAP_U / 31, (I.describe(inst), eU)
        assert eL is None or (np.isfinite(eL) and eL <= I.CAP_L / 31), (I.describe(inst), eL)
        assert (inst.sR or inst.vR) >= 1e3, I.describe(inst)  # still ill-conditioned by two orders beyond the 30x rule
    assert len(dropped) <= 2, dropped  # the condition is the exception: a batch that needs it often is not the batch the issue describes


@pytest.mark.parametrize("m1,m2", [(50, 25), (300, 80)])
def test_two_axis_batches_leave_the_cap_alone(m1, m2):
    """axis = "both" (the launchers' batches): at most one axis at 1e6, see ill_grids.BOTH_RATIOS."""
    c = I.cfg(4)
    insts = [i for turn in (0, 1, 2) for i in I.batch(m1, m2, 6, "both", turn)]
    assert {(i.sR, i.vR) for i in insts} >= {(1e4, 1e4), (1e6, 1e4)}
    admitted = I.admit(c, tuple(insts))
    print("%dx%d both axes: %d of %d with a dropped ratio" % (m1, m2, sum(a != b for a, b in zip(insts, admitted)), len(insts)))
    for inst in admitted:
        eU = I.oracle_distance(c, inst)[0]
        assert np.isfinite(eU) and eU <= I.CAP_U / 31, (I.describe(inst), eU)
        assert min(inst.sR, inst.vR) >= 1e3, I.describe(inst)


@pytest.mark.parametrize("m1,m2", [(50, 25), (128, 64), (600, 40), (1100, 20), (40, 600)])
def test_construction_on_every_raw_interval(m1, m2):
    """Both sides and both ratios on every raw interval of both axes: strictly increasing, every interval >= 1e-8, realised ratio
    >= R / 2, the inserted node found once (asserted inside s_grid / v_grid) -- and the other intervals are the raw grid's."""
    K = 100.0
    raw_s, raw_v = I.raw_s(m1, K), I.raw_v(m2)
    for side in I.SIDES:
        for R0 in I.RATIOS:
            for i in range(m1 - (0 if side == "lower" else 1)):
                R = I.fit_ratio(raw_s[i + 1] - raw_s[i], R0)
                vs, ds, x = I.s_grid(m1, K, i, R, side)
                assert np.array_equal(np.delete(vs, i + 1), raw_s[:-1]) and vs[i + 1] == x
            for j in range(m2 - (0 if side == "lower" else 1)):
                R = I.fit_ratio(raw_v[j + 1] - raw_v[j], R0)
                vv, dv, x = I.v_grid(m2, j, R, side)
                assert np.array_equal(np.delete(vv, j + 1), raw_v[:-1]) and vv[j + 1] == x


def test_turns_give_every_position_both_ratios_and_the_other_axis_is_well_conditioned():
    for m1, m2 in ((50, 25), (300, 80), (600, 40)):
        for axis in ("s", "v"):
            n = len(I.s_positions(m1, 100.0)) if axis == "s" else len(I.v_positions(m2, 11))
            seen = {}
            for turn in (0, 1):
                for inst in I.batch(m1, m2, n, axis, turn, 11 if axis == "v" else None):
                    g = I.grids(inst)
                    name = inst.sname if axis == "s" else inst.vname
                    seen.setdefault(name, []).append((inst.sR or inst.vR, inst.s_side or inst.v_side))
                    assert Cm.interval_ratios(g[3 if axis == "s" else 2])[0] <= Cm.COND_MAX
                    assert Cm.interval_ratios(g[2 if axis == "s" else 3])[0] >= (inst.sR if axis == "s" else inst.vR) / 2
            assert len(seen) == n and all(len(v) == 2 for v in seen.values()), seen
            for name, ((Ra, sa), (Rb, sb)) in seen.items():
                # (on the v-axis a ratio of 1e6 drops where it must to keep every interval >= 1e-8, as far as 1e4 on the first interval)
                assert sa != sb and min(Ra, Rb) == 1e4 and (max(Ra, Rb) == 1e6 or axis == "v"), (name, seen[name])


def test_yard_is_deterministic_and_covers_the_siblings():
    c = I.cfg(3)
    inst = I.batch(50, 25, 5, "s", 0)[3]
    sib = I.siblings(inst)
    assert len(sib) == 2 and {x.si for x in sib} == {inst.si - 1, inst.si + 1} and all((x.sR, x.s_side) == (inst.sR, inst.s_side) for x in sib)
    y1 = I.yard(c, inst)
    I.oracle_distance.cache_clear()
    I.exact.cache_clear()
    assert I.yard(c, inst) == y1
    assert y1[0] == max(I.oracle_distance(c, x)[0] for x in [inst] + sib) and y1[1] is None
    first = I.batch(50, 25, 5, "s", 0)[0]
    assert first.si == 0 and len(I.siblings(first)) == 1  # (nothing below the first interval)


# ---- the rule on synthetic triples ----------------------------------------------------------------------------------------
def _triple(e_h, e_o):
    """(U, U_o, U_x) with max|U_x| = 1, |U - U_x| = e_h and |U_o - U_x| = e_o at opposite signs on one node."""
    Ux = np.linspace(0.0, 1.0, 11)
    U, Uo = Ux.copy(), Ux.copy()
    U[5] += e_h
    Uo[5] -= e_o
    return U, Uo, Ux


def _never():
    raise AssertionError("the adjudicator must not be called")


def test_judge_in_band():
    U, Uo, Ux = _triple(3e-11, 3e-11)
    v = I.judge(U, Uo, _never, _never)
    assert v["ok"] and v["stage"] == "band" and abs(v["d"] - 6e-11) < 1e-15


def test_judge_out_of_band_within_30x():
    U, Uo, Ux = _triple(2.9e-7, 1e-8)
    v = I.judge(U, Uo, lambda: (Ux, None), lambda: (1e-8, None))
    assert v["ok"] and v["stage"] == "adjudicated" and abs(v["ratio"] - 29) < 1e-3 and abs(v["e_o"] - 1e-8) < 1e-15
    # the floor: a yardstick of nothing still admits 1e-11
    U, Uo, Ux = _triple(9e-12, 2e-10)
    assert I.judge(U, Uo, lambda: (Ux, None), lambda: (0.0, None))["ok"]
    # the larger sibling is the yardstick, not the instance's own e_o
    U, Uo, Ux = _triple(2.9e-7, 1e-9)
    assert I.judge(U, Uo, lambda: (Ux, None), lambda: (1e-8, None))["ok"]


def test_judge_out_of_band_beyond_30x():
    U, Uo, Ux = _triple(3.1e-7, 1e-8)
    v = I.judge(U, Uo, lambda: (Ux, None), lambda: (1e-8, None))
    assert not v["ok"] and v["stage"] == "adjudicated" and v["ratio"] > 30
    # lambda_bar alone beyond 30x fails the instance
    lam_x = np.zeros(11)
    lam, lo = lam_x.copy(), lam_x.copy()
    lam[2], lo[2] = 4e-6, -1e-7
    U, Uo, Ux = _triple(1e-12, 1e-12)
    v = I.judge(U, Uo, lambda: (Ux, lam_x), lambda: (1e-12, 1e-7), lam, lo)
    assert not v["ok"] and v["stage"] == "adjudicated" and v["l_h"] > 30 * v["lyard"]
    lam[2] = 2.9e-6
    assert I.judge(U, Uo, lambda: (Ux, lam_x), lambda: (1e-12, 1e-7), lam, lo)["ok"]
    # beyond the sanity cap nothing is adjudicated
    U, Uo, Ux = _triple(2e-4, 0.0)
    v = I.judge(U, Uo, _never, _never)
    assert not v["ok"] and v["stage"] == "cap"


def test_judge_non_finite():
    U, Uo, Ux = _triple(0.0, 0.0)
    U[3] = np.nan
    v = I.judge(U, Uo, _never, _never)
    assert not v["ok"] and v["stage"] == "finite"
    U, Uo, Ux = _triple(0.0, 0.0)
    lam = np.zeros(11)
    lam[0] = np.inf
    assert I.judge(U, Uo, _never, _never, lam, np.zeros(11))["stage"] == "finite"


def test_judge_value_is_the_field_rule_at_one_node():
    v = I.judge_value(10.0 + 5e-10, 10.0, 100.0, _never, _never)
    assert v["ok"] and v["stage"] == "band" and abs(v["d"] - 5e-12) < 1e-15
    assert I.judge_value(np.nan, 10.0, 100.0, _never, _never)["stage"] == "finite"
    assert I.judge_value(10.02, 10.0, 100.0, _never, _never)["stage"] == "cap"
    v = I.judge_value(10.0 + 2.9e-5, 10.0 - 1e-6, 100.0, lambda: (10.0, 100.0), lambda: 1e-8)
    assert v["ok"] and v["stage"] == "adjudicated" and abs(v["ratio"] - 29) < 1e-6
    assert not I.judge_value(10.0 + 3.1e-5, 10.0 - 1e-6, 100.0, lambda: (10.0, 100.0), lambda: 1e-8)["ok"]
