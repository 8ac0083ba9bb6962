"""CPU-only: the numpy reference of the sampled ladder (tests/samples_ref.py) and the two claims the strike surface stands on,
checked on the oracle:
  - the reference is exact to round-off on cubics in s on a non-uniform grid, at both clamped ends, and a node hit is the node;
  - homogeneity: the solve on the grid scaled by a = K'/K is a U_K node by node, |U_scaled - a U| <= 1e-12 max|U| (measured:
    6e-15 on 50x25x20, 1.4e-14 on 100x50x40), for calls with r_f = 0 and for puts;
  - the surface strike_samples builds from ONE field differs from the per-strike grids' prices by less than the per-strike price
    at K differs between the (m1, m2) and the (2 m1, 2 m2) grid: it stays inside the grid's own discretisation error."""
import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import sample_cases as SC
import samples_ref as R
import pde_based_heston_solver_gpu_accelerated_amd.solver as Sv

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
K_BASE = 100.0
STRIKES = [80.0 + 5.0 * k for k in range(10)]  # 80 .. 125


def test_cubics_are_reproduced_at_every_kind_of_spot():
    rng = np.random.default_rng(7)
    s = np.cumsum(rng.uniform(0.2, 3.0, 41))  # non-uniform, 40 intervals
    vv = np.array([0.0, 0.04, 0.1])
    cubic = lambda x: 0.3 * x ** 3 - 2.0 * x ** 2 + 5.0 * x - 7.0
    U = np.concatenate([np.zeros(41), cubic(s), np.ones(41)])  # row 1 is the row of V_0 = 0.04
    spots = R.kernel_test_spots(s, s[20])
    val, amp, flags = R.sample_field(U, s, vv, 0.04, spots, scales=np.full(10, 1.7))
    assert (flags == 0).all()
    scale = np.abs(cubic(s)).max()
    assert np.abs(val - 1.7 * cubic(spots)).max() <= 64 * np.finfo(float).eps * amp.max() * scale
    # the clamped ends use the first and the last four nodes
    assert list(R.taps(s, spots[8])[0]) == [0, 1, 2, 3] and list(R.taps(s, spots[9])[0]) == [37, 38, 39, 40]
    # the interior stencil has one node below the bracketing interval and two above its lower end
    i = 13
    assert list(R.taps(s, s[i] + 0.5 * (s[i + 1] - s[i]))[0]) == [i - 1, i, i + 1, i + 2]


def test_node_hit_is_the_node_and_off_grid_is_nan():
    s = np.linspace(1.0, 9.0, 17)
    vv = np.array([0.0, 0.5])
    U = np.arange(34, dtype=np.float64) ** 1.5
    val, amp, flags = R.sample_field(U, s, vv, 0.5, [s[4], s[4] + 5e-11, s[0], s[16], 0.999, 9.001, np.nan])
    assert val[0] == U[17 + 4] and val[1] == U[17 + 4] and val[2] == U[17] and val[3] == U[33]
    assert list(flags) == [0, 0, 0, 0, R.OFF_GRID, R.OFF_GRID, R.OFF_GRID] and np.isnan(val[4:]).all()
    # V_0 off the v-grid: row 0
    assert R.sample_field(U, s, vv, 0.3, [s[4]])[0][0] == U[4]
    # a zero interval inside the stencil: degenerate
    s2 = s.copy()
    s2[6] = s2[5]
    assert R.sample_field(U, s2, vv, 0.5, [0.5 * (s2[6] + s2[7])])[2][0] == R.DEGENERATE


@pytest.mark.parametrize("name,grid,cases", SC.LOCATE_EDGES, ids=[e[0].split(":")[0].replace(" ", "_") for e in SC.LOCATE_EDGES])
def test_the_reference_on_the_locate_edges(name, grid, cases):
    """The reference is not its own judge: sample_cases.LOCATE_EDGES states, by hand from include/hadi.h, what every spot is (the
    node hit, the stencil's first node, off grid, degenerate); the weights of an interior spot are pinned by what they must do --
    sum to 1 and reproduce the cubic through the four nodes' own values."""
    s = np.array(grid)
    for x, want in cases:
        idx, w, flag = R.taps(s, x)
        if want[0] == "hit":
            assert flag == 0 and list(idx) == [want[1]] * 4 and list(w) == [1.0, 0.0, 0.0, 0.0], (name, x)
        elif want[0] == "interior":
            assert flag == 0 and list(idx) == list(range(want[1], want[1] + 4)), (name, x, idx)
            assert np.isfinite(w).all() and abs(w.sum() - 1.0) <= 8 * np.finfo(float).eps * np.abs(w).sum(), (name, x, w)
            for p in (1, 2, 3):  # (monomials about the spot: sum_a w_a (s_a - x)^p = 0 for every polynomial degree <= 3)
                t = w * (s[idx] - x) ** p
                assert abs(t.sum()) <= 16 * np.finfo(float).eps * np.abs(t).sum(), (name, x, p)
        else:
            assert flag == (R.OFF_GRID if want[0] == "off" else R.DEGENERATE) and (idx == -1).all(), (name, x, flag)
    # through sample_field: a flagged entry is NaN and leaves the flags and values of the call's other entries alone
    m1 = s.size - 1
    U = np.arange(3 * (m1 + 1), dtype=np.float64) + 1.0
    val, _, flags = R.sample_field(U, s, np.array([0.0, 0.04, 0.1]), 0.04, [x for x, _ in cases])
    for q, (x, want) in enumerate(cases):
        assert flags[q] == {"hit": 0, "interior": 0, "off": R.OFF_GRID, "deg": R.DEGENERATE}[want[0]]
        assert np.isnan(val[q]) == (want[0] in ("off", "deg"))
        if want[0] == "hit":
            assert val[q] == U[m1 + 1 + want[1]]


def test_domain_spots_name_their_entries_by_the_definition():
    """sample_cases.domain_spots on a real grid: the tolerance block against the inequalities of include/hadi.h, written out."""
    vs = SC.oracle_batch(50, 25, 1)[1][0]
    spots, scales, kinds = SC.domain_spots(vs, Cm.S_0)
    m1 = 50
    assert spots.size <= 4 * m1 + 16 and kinds[0] == SC.S0 and spots[0] == Cm.S_0 and 0.0 < vs[0] < 1e-13
    tol = spots[kinds >= SC.TOL_HIT]
    t = int(np.argmin(np.abs(vs - tol[0])))
    assert 1.0 <= vs[t] <= 200.0 and list(tol) == [vs[t] - 5e-11, vs[t] + 5e-11, vs[t] - 2e-10, vs[t] + 2e-10, 0.0, -5e-11, vs[m1] + 5e-11]
    assert [abs(x - vs[t]) < 1e-10 for x in tol[:4]] == [True, True, False, False]
    assert tol[4] < vs[0] and tol[5] < vs[0] and tol[6] > vs[m1] and abs(tol[5] - vs[0]) < 1e-10 and abs(tol[6] - vs[m1]) < 1e-10
    assert list(R.taps(vs, tol[2])[0]) == list(range(t - 2, t + 2)) and list(R.taps(vs, tol[3])[0]) == list(range(t - 1, t + 3))
    # one interior spot in every interval, and in the six intervals at the clamp the stencils the clamp gives
    first = {int(np.searchsorted(vs, x)) - 1 for x in spots[kinds == SC.INTERIOR]}
    assert first == set(range(m1))
    for i, i0 in ((0, 0), (1, 0), (2, 1), (m1 - 3, m1 - 4), (m1 - 2, m1 - 3), (m1 - 1, m1 - 3)):
        x = [x for x in spots[kinds == SC.INTERIOR] if vs[i] < x < vs[i + 1]][0]
        assert R.taps(vs, x)[0][0] == i0


def _solve(m1, m2, N, vs, vv, ds, dv, U0, put_strikes=None):
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.0, *MODEL, O.EU,
                      option_type=O.PUT if put_strikes is not None else O.CALL, strikes=put_strikes)
    return O.solve_batch(p, vs, vv, ds, dv, U0)[0]


_BASE = {}


def _base_field(m1, m2, N, put):
    """The field of the base strike on its own grid: computed once, left unchanged."""
    key = (m1, m2, N, put)
    if key not in _BASE:
        vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, [K_BASE])
        if put:
            U0 = Cm.put_payoff(vs, [K_BASE], m2)
        _BASE[key] = (vs, vv, ds, dv, _solve(m1, m2, N, vs, vv, ds, dv, U0, [K_BASE] if put else None))
    return _BASE[key]


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
@pytest.mark.parametrize("m1,m2,N", [(50, 25, 20), (100, 50, 40)], ids=["50x25x20", "100x50x40"])
def test_oracle_homogeneity(m1, m2, N, put):
    vs, vv, ds, dv, U = _base_field(m1, m2, N, put)
    a = np.array(STRIKES).reshape(-1, 1) / K_BASE
    n = len(STRIKES)
    vs_a, ds_a = vs * a, ds * a  # the grid scaled by a, instance by instance
    vv_a, dv_a = np.repeat(vv, n, 0), np.repeat(dv, n, 0)
    U0 = Cm.put_payoff(vs_a, STRIKES, m2) if put else np.tile(np.maximum(vs_a - np.array(STRIKES).reshape(-1, 1), 0.0), (1, m2 + 1))
    Ua = _solve(m1, m2, N, np.ascontiguousarray(vs_a), np.ascontiguousarray(vv_a), np.ascontiguousarray(ds_a),
                np.ascontiguousarray(dv_a), np.ascontiguousarray(U0), STRIKES if put else None)
    worst = np.abs(Ua - a * U).max() / np.abs(U).max()
    print("homogeneity %dx%dx%d %s: worst |U_scaled - a U| / max|U| = %.2e" % (m1, m2, N, "put" if put else "call", worst))
    assert worst <= 1e-12


def _node_price(m1, m2, N, K):
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, [K])
    U = _solve(m1, m2, N, vs, vv, ds, dv, U0)
    return U[0, O.find_s_index(vs[0], Cm.S_0) + O.find_v_index(vv[0], Cm.V_0) * (m1 + 1)]


def test_one_sweep_surface_stays_inside_the_discretisation_error():
    m1, m2, N = 50, 25, 20
    vs, vv, ds, dv, U = _base_field(m1, m2, N, False)
    spots, scales = Sv.strike_samples(Cm.S_0, K_BASE, STRIKES)
    surf, amp, flags = R.sample_field(U[0], vs[0], vv[0], Cm.V_0, spots, scales)
    assert (flags == 0).all() and amp.max() <= 2.0 * scales.max()
    per_strike = np.array([_node_price(m1, m2, N, K) for K in STRIKES])
    worst = np.abs(surf - per_strike).max()
    own = abs(_node_price(m1, m2, N, K_BASE) - _node_price(2 * m1, 2 * m2, N, K_BASE))
    print("surface vs per-strike grids: worst %.3e; the grid's own error at K (50x25 vs 100x50): %.3e" % (worst, own))
    assert surf[STRIKES.index(K_BASE)] == per_strike[STRIKES.index(K_BASE)]  # the base strike is a node hit with scale 1
    assert worst < own
