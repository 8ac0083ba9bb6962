"""CPU checks of the test-side Greeks reference (tests/greeks_ref.py) itself: the derivative operators are exact on quadratics
at every node, the ladder's node row is the three-weight formula, lambda_bar marks the exercise region of the oracle's American
fields, and every call case of the GPU and emulator tests carries a node with a boundary-vector entry on its ladder row."""
import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import greeks_ref as G


@pytest.mark.parametrize("seed,m", [(1, 2), (2, 3), (3, 7), (4, 50), (5, 257)])
def test_D1_D2_exact_on_quadratics_at_every_node(seed, m):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(0.05, 2.0, m + 1))
    for _ in range(5):
        c0, c1, c2 = rng.uniform(-3, 3, 3)
        f = c0 + c1 * x + c2 * x * x
        scale = np.abs(f).max() * max(np.abs(G.D1(x)).sum(axis=1).max(), np.abs(G.D2(x)).sum(axis=1).max())
        assert np.abs(G.D1(x) @ f - (c1 + 2 * c2 * x)).max() <= 1e-14 * scale
        assert np.abs(G.D2(x) @ f - 2 * c2).max() <= 1e-14 * scale


def test_D1_D2_on_the_oracle_grids():
    vs, vv, ds, dv, _ = Cm.oracle_grids(256, 128, [100.0])
    for x in (vs[0], vv[0]):
        f = 0.3 - 0.7 * x + 0.011 * x * x
        assert np.abs(G.D1(x) @ f - (-0.7 + 0.022 * x)).max() <= 1e-9
        assert np.abs(G.D2(x) @ f - 0.022).max() <= 1e-7
        assert np.array_equal(G.D2(x)[0], G.D2(x)[1]) and np.array_equal(G.D2(x)[-1], G.D2(x)[-2])


@pytest.mark.parametrize("variant,put", [("EU", False), ("AM", True)])
def test_node_row_is_the_three_weight_formula(variant, put):
    m1, m2, N = 50, 25, 8
    vs, vv, ds, dv, U0, inst = G.oracle_instances(m1, m2, [100.0], [N], [Cm.T / N], variant, put=put)
    I = inst[0]
    j0, i0 = G.find_node(vv[0], Cm.V_0), G.find_node(vs[0], Cm.S_0)
    assert i0 > 0 and j0 > 0
    lad = G.ladder(I["p"], vs[0], vv[0], ds[0], dv[0], I["U"], I["lam"], j0, I["b"])
    U = I["U"].reshape(m2 + 1, m1 + 1)
    s, v = vs[0], vv[0]
    a, b = s[i0] - s[i0 - 1], s[i0 + 1] - s[i0]
    c, d = v[j0] - v[j0 - 1], v[j0 + 1] - v[j0]
    bs = np.array([-b / (a * (a + b)), (b - a) / (a * b), a / (b * (a + b))])
    bv = np.array([-d / (c * (c + d)), (d - c) / (c * d), c / (d * (c + d))])
    gs = np.array([2 / (a * (a + b)), -2 / (a * b), 2 / (b * (a + b))])
    gv = np.array([2 / (c * (c + d)), -2 / (c * d), 2 / (d * (c + d))])
    blk = U[j0 - 1:j0 + 2, i0 - 1:i0 + 2]
    want = [U[j0, i0], bs @ blk[1], gs @ blk[1], bv @ blk[:, 1], gv @ blk[:, 1], bv @ blk @ bs]
    scale = np.abs(blk).max() * max(np.abs(gs).sum(), np.abs(gv).sum(), np.abs(bs).sum() * np.abs(bv).sum())
    assert np.abs(lad[i0, :6] - want).max() <= 1e-13 * scale
    assert lad[i0, G.PRICE] == U[j0, i0]
    assert G.NAMES[G.THETA] == "theta" and len(G.NAMES) == 8


@pytest.mark.parametrize("variant", ["AM", "AM_DIV"])
def test_lambda_marks_the_exercise_region(variant):
    m1, m2, N = 100, 50, 100
    vs, vv, ds, dv, U0, inst = G.oracle_instances(m1, m2, [100.0], [N], [Cm.T / N], variant, put=True)
    I = inst[0]
    j0 = G.find_node(vv[0], Cm.V_0)
    lad = G.ladder(I["p"], vs[0], vv[0], ds[0], dv[0], I["U"], I["lam"], j0, I["b"])
    pay = U0[0].reshape(m2 + 1, m1 + 1)[j0]
    ex = lad[:, G.LAMBDA] > 0
    assert ex.any() and not ex.all()
    # lambda_bar > 0 exactly where U == U_0; pay > 0 leaves out the far nodes where the put's payoff and its value are both 0
    # (U == U_0 there without any exercise)
    assert np.array_equal(ex, (lad[:, G.PRICE] == pay) & (pay > 0))
    # theta: the semi-discrete residual is ~0 deep inside the exercise region and O(1) at worst next to the boundary
    # (American put, 100 steps: largest value over the exercised nodes 0.17, median 5e-11)
    assert np.abs(lad[ex, G.THETA]).min() < 1e-6 and np.abs(lad[ex, G.THETA]).max() < 5.0


@pytest.mark.parametrize("m1,m2,col", [(50, 25, 42), (256, 128, 217), (512, 256, 434)])
def test_call_ladder_rows_carry_a_boundary_entry(m1, m2, col):
    """b != 0 on exactly one node of the ladder row of V_0 (the reference's b1 quirk: column m1 - j0), so the b e_N term of
    theta is exercised by every call case."""
    N = 2
    strikes = Cm.well_conditioned_strikes(m1, 1)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes, Cm.v0_for(m2))
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=0.007)
    b, _, _ = G.boundary_vector(p, vs[0], vv[0], ds[0], dv[0], U0[0])
    j0 = G.find_node(vv[0], Cm.v0_for(m2))
    row = b.reshape(m2 + 1, m1 + 1)[j0]
    assert list(np.nonzero(row)[0]) == [col] and col == m1 - j0
