"""CPU-only: tests/jumps_ref.py's generator -- the formula of hadi_jump_entry_value -- against the same generator in 40-digit
arithmetic (tests/jumps_exact.py, mpmath), on the widths and laws of tests/jump_cases.py.

Well-conditioned grids (asserted): every checked entry within the suite's entry bound 1e-13 max(1, |kbar| s_i / min h).  All rows
up to m1 = 129, the rows of jump_cases.matrix_rows above.  Measured: worst 0.24 of the bound (m1 = 129, law (-0.1, 0.15)).

Ill-conditioned grids (one interval 1e6 times shorter than its neighbour, every placement of ill_grids.s_positions): the ENTRIES of
the two columns around the tiny interval are up to 2e4 times over the entry bound (absolute errors up to 2.4e-7: a (dPhi) + b s_i
(1 + kbar) (dPhi') with a, b ~ 1 / h), so the entry bound is not asserted there.  What a price feels is asserted instead:
  * the sum of the two entries around the tiny interval against the 40-digit sum, at the row's entry bound: their errors cancel
    (measured 0.025 of the bound);
  * G u on the call and the put payoff against 40 digits, at 1e-13 of |G| |u| -- taken over the field, max_i (|G| |u|)_i, and row by
    row on every row that carries 1e-6 of that maximum (measured 3.8e-16 and 4.3e-14).  Row by row WITHOUT that floor the figure is
    2.9e-12 at m1 = 50 and 2.2e-11 at m1 = 600, on rows whose whole action is a far tail (|G| |u| = 1e-19 .. 1e-250 at d = 9 .. 34):
    the relative error of Phi's tail grows like d^2 u in any fp64 evaluation, and a value of 1e-19 moves no price;
  * |G 1| and |G s| at 1e-12 max s, as tests/test_gpu_jumps.py has them (measured 0.73 of the bound below).
The sum and the row sums carry one more term, the round-off of the STORED entries themselves: gamma(20) times the magnitudes
involved (jump_cases.ENTRY_OPS: an entry is the result of at most 20 rounded operations), the sums taken in np.longdouble so that
the check adds none of its own.  Without it no fp64 matrix can pass on these grids: beside the tiny interval the compensator's
entries are kbar s_i / h = 2e7, their half-ulp times s = 100 is 4e-7 against 1e-12 max s = 8e-10; and with the tiny interval LAST
the two columns carry the linear continuation beyond s_max with slope 1 / h, entries of 1e6 whose half-ulps alone move their sum by
1e-10 against a bound of 1e-13 (measured there: the sum at 800 times the entry bound, at 0.39 of the bound with the term; for an
interior tiny interval the plain entry bound is asserted as well).  On well-conditioned grids the term is below 1e-13.

The per-row distances of the numpy formula from 40 digits on the ill grids are the yardstick of the device tests
(tests/golden/jump_exact_ill.json, tools/record_jump_exact.py); the placements this file computes are compared with the fixture."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import jump_cases as JC
import jumps_exact as JX
import jumps_ref as JR

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble


def laws_at(m1):
    """All laws on the small widths; two of them, rotating with the width, from 63 on (a row costs m1 40-digit erfc)."""
    if m1 <= 50:
        return JC.LAWS
    k = JC.M1_EDGES.index(m1)
    return (JC.LAWS[k % len(JC.LAWS)], JC.LAWS[(k + 3) % len(JC.LAWS)]) if m1 <= 129 else (JC.LAWS[k % len(JC.LAWS)],)


@pytest.mark.parametrize("m1", sorted(JC.M1_EDGES + (50,)))
def test_numpy_generator_on_well_conditioned_grids(m1):
    K = Cm.well_conditioned_strikes(m1, 1)[0]
    g = O.grid(m1, 8 * K, Cm.S_0, K, K / 5, 8, 5.0, Cm.V_0, 5.0 / 500)
    vs = g[0]
    assert Cm.interval_ratios(g[2])[0] <= Cm.COND_MAX
    rows = JC.matrix_rows(m1)
    assert (m1 > 129 or rows == list(range(1, m1 + 1))) and len(rows) <= max(32, m1)
    for mu, sig in laws_at(m1):
        X = JX.generator_rows(vs, mu, sig, rows)
        Gr = JR.generator(vs, mu, sig)
        b = JC.entry_bound(vs, mu, sig)
        worst = max((np.abs(Gr[i] - JX.as_float(X[i])) / b[i]).max() for i in rows)
        print("m1 = %d (%g, %g), %d rows: worst entry at %.3f of its bound" % (m1, mu, sig, len(rows), worst))
        assert worst <= 1.0, (m1, mu, sig, worst)


def ill_laws(m1, p):
    return JC.ILL_LAWS if m1 <= 129 else (JC.ILL_LAWS[p % len(JC.ILL_LAWS)],)


def ill_measure(vs, tiny, law, rows):
    """(per-row distance of the numpy entries from 40 digits, per-row distance of the two-column sum, the 40-digit rows)."""
    X = JX.generator_rows(vs, law[0], law[1], rows)
    Gr = JR.generator(vs, *law)
    dist = [float(np.abs(Gr[i] - JX.as_float(X[i])).max()) for i in rows]
    sums = [abs(float((LD(Gr[i, tiny]) + LD(Gr[i, tiny + 1])) - LD(float(X[i][tiny] + X[i][tiny + 1])))) for i in rows]
    return dist, sums, X, Gr


ILL_CASES = [(m1, p) for m1, _ in JC.ILL_SHAPES for p in range(len(JC.ill_s_grids(m1)[0]))]


@pytest.mark.parametrize("m1,p", ILL_CASES, ids=["%d-%s" % (m1, JC.ill_s_grids(m1)[0][p][0].replace(" ", "_")) for m1, p in ILL_CASES])
def test_numpy_generator_on_ill_grids(m1, p):
    places, K = JC.ill_s_grids(m1)
    name, vs, ds, tiny = places[p]
    rows = JC.ill_rows(m1, tiny)
    fix = json.load(open(os.path.join(HERE, "golden", JC.ILL_FIXTURE)))["cases"]
    for law in ill_laws(m1, p):
        dist, sums, X, Gr = ill_measure(vs, tiny, law, rows)
        b = JC.entry_bound(vs, *law)
        rec = fix[JC.ill_key(m1, name, law)]
        assert rec["rows"] == rows and np.allclose(rec["dist"], dist, rtol=1e-6, atol=1e-30) and np.allclose(rec["sum_dist"], sums, rtol=1e-6, atol=1e-30)
        A = np.abs(Gr).astype(LD)
        # the two columns around the tiny interval
        rep = JC.gamma(JC.ENTRY_OPS) * (np.abs(Gr[rows, tiny]) + np.abs(Gr[rows, tiny + 1]))
        r_sum = float((np.array(sums) / (b[rows] + rep)).max())
        r_sum_plain = float((np.array(sums) / b[rows]).max())
        worst_rs = JC.row_sums_ratio(Gr, vs, JC.ENTRY_OPS)  # the row sums, in np.longdouble
        # the action on the two payoffs
        worst_f = worst_r = worst_all = 0.0
        for u in (np.maximum(vs - K, 0.0), np.maximum(K - vs, 0.0)):
            ex = np.array([JX.action(X[i], u) for i in rows])
            got = (Gr[rows].astype(LD) @ u.astype(LD)).astype(np.float64)
            sc = (A[rows] @ np.abs(u).astype(LD)).astype(np.float64)
            err = np.abs(got - ex)
            assert (err[sc == 0.0] == 0.0).all()  # (rows with |G| |u| = 0: compared absolutely)
            worst_f = max(worst_f, err.max() / sc.max())
            heavy = sc >= 1e-6 * sc.max()
            worst_r = max(worst_r, (err[heavy] / sc[heavy]).max())
            worst_all = max(worst_all, (err[sc > 0] / sc[sc > 0]).max())
        print("m1 = %d, %s, (%g, %g): entries %.0f x their bound (abs %.2e); two-column sum %.3f of its bound (%.1f without the "
              "stored entries' round-off); action %.2e of max |G||u|, %.2e row by row on the rows that carry weight (%.2e on all); "
              "row sums %.3f of their bound" % (m1, name, law[0], law[1], (np.array(dist) / b[rows]).max(), max(dist), r_sum, r_sum_plain,
                                                worst_f, worst_r, worst_all, worst_rs))
        assert r_sum <= 1.0 and worst_rs <= 1.0 and worst_f <= 1e-13 and worst_r <= 1e-13, (name, law)
        if name != "last interval":  # (an interior tiny interval: the plain entry bound holds for the sum)
            assert r_sum_plain <= 1.0, (name, law, r_sum_plain)
