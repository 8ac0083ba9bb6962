"""The Bates sub-step on the device over its admitted domain (tests/jump_cases.py), judged IN ISOLATION: with N = 1 the plain call on
the same route leaves the field P in front of the sub-step (the zero-intensity identity, asserted bit for bit by
tests/test_gpu_jumps.py), the Bates call leaves U behind it, hadi_debug_jump_matrix returns the matrix G_dev the product multiplies
with, and D = U - P is held to R = a (P @ G_dev^T) formed in np.longdouble at the derived bound of a K-term inner product
(jump_cases.substep_ratio).  The field is rough (asserted on P), the laws fill the whole matrix, a = lambda dt is 1 (the admitted
edge) and 0.37, and every instance of a batch has its own grid and law.  Shapes: every m1 at which hadi_pick_shape changes the
layout, a layout full and nearly empty, m1 = 2 and 1024; every row count around the 64-row pass and its 16-row wavefront tiles, 4
and 528; a shared matrix with several instances per staged strip; s-grids with one interval 1e6 times shorter than its neighbour.
The matrix itself is held to the numpy generator (which tests/test_jumps_exact.py holds to 40 digits): on well-conditioned grids at
the entry bound, on the ill grids row by row at max(entry bound, 30 x the numpy formula's own recorded distance from 40 digits).
Launches that do not start at instance 0: "streams" = 2 cuts a batch in two halves; both halves equal the one-stream call bit for bit
and keep the reference's bounds.  Wide laws over four steps against tests/jumps_ref.py at 1e-10, on inputs that keep the explicit
compensator from amplifying round-off (asserted).

Measured on the MI355X (worst over the cases of each test; every figure is printed):
  the product, |D - R| over its bound: 0.063 over the m1 and m2 edges (worst: 50x527), 0.027 with the shared matrix, 0.088 on the ill
    grids; one entry moved by 1e-9 of its row's maximum: 60 (last K tile, m1 = 1024) to 1.7e6 (far pair) times the bound;
  the matrix on well-conditioned grids: 0.61 of the entry bound (m1 = 511, law (-0.1, 0.15)), ocml's erfc and log included;
  the matrix on ill grids (R = 1e6), of the four bounds of jump_cases.ill_matrix_check: entries 0.17, two-column sum 0.053, action on
    the payoffs 0.004, row sums 0.68;
  two streams: fields and Jacobians bit-equal to one stream; field 1.1e-12 of max|U_ref|, prices 1.1e-14, J 5.3e-8;
  wide laws over four steps: 7.1e-15 (50x25) and 1.7e-13 (300x12) of max|U_ref|.
"""
import json
import os

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm
import jump_cases as JC
import jumps_ref as JR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "streams": 0, "jump_share": 1}
LD = np.longdouble


class tuned:
    """Tuning keys for the block; every one goes back to its default on the way out (the handle is the session's)."""

    def __init__(self, sv, tuning):
        self.sv, self.tuning = sv, tuning

    def __enter__(self):
        for k, v in self.tuning.items():
            self.sv.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.tuning:
            self.sv.set_tuning(k, DEFAULTS[k])


def grid_batch(vs, ds, m2):
    """A GridViewsBatch of the s-grids vs [n][m1 + 1] with the well-conditioned v-grid of m2 on every instance."""
    n = vs.shape[0]
    vv, dv = JC.v_grid(m2)
    g = object.__new__(H.GridViewsBatch)
    g.m1, g.m2, g.n = vs.shape[1] - 1, m2, n
    g.Vec_s, g.Delta_s = np.ascontiguousarray(vs), np.ascontiguousarray(ds)
    g.Vec_v, g.Delta_v = np.ascontiguousarray(np.tile(vv, (n, 1))), np.ascontiguousarray(np.tile(dv, (n, 1)))
    return g


def isolate(solver, name, m1, m2, vs, ds, mu, sig, seed, shared=False, perturb=None):
    """One step with dt = 1e-6 on the streaming route, plain and with jumps -> (P, U, the matrices, the weights); the route, the
    roughness of P and the rule are asserted here."""
    n = vs.shape[0]
    grids = grid_batch(vs, ds, m2)
    U0 = JC.rough_field(seed, vs, m2)
    lam = np.array([JC.intensity(JC.WEIGHTS[k % 2]) for k in range(n)])
    avec = lam * JC.DT  # (as the library forms the weight)
    assert avec[0] == 1.0 and (avec <= 1.0).all()
    head = (m1, m2, 1, JC.DT, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (grids,)
    with tuned(solver, STREAMING):
        P = solver.DO_timestepping(*head, U0.copy())
        d0 = solver.describe_last_sweep()
        U = solver.bates_timestepping(*head, U0.copy(), lam, mu, sig, shared_grid=shared)
        d1 = solver.describe_last_sweep()
    assert d1.endswith(JUMP_WORDS) and d1[:-len(JUMP_WORDS)] == d0, (d0, d1)  # the same passes in front of the Bates clause
    rough = min(JC.roughness(P[k], m1, m2) for k in range(n))
    assert rough >= 0.1, (name, rough)
    worst = 0.0
    mats = {}
    for k in range(n):
        key = 0 if shared else k
        if key not in mats:
            mats[key] = solver.debug_jump_matrix(vs[key], float(np.ravel(mu)[key] if np.ndim(mu) else mu), float(np.ravel(sig)[key] if np.ndim(sig) else sig))
        r, at = JC.substep_ratio(P[k], U[k], mats[key], avec[k], m1, m2)
        assert not np.array_equal(U[k], P[k])
        worst = max(worst, r)
        assert r <= 1.0, (name, k, r, at)
    print("%s %dx%d x%d: worst |D - R| at %.3f of its bound; P rough to %.2f" % (name, m1, m2, n, worst, rough))
    return P, U, mats, avec


# ---- item 1: the product in isolation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", JC.M1_EDGES)
def test_substep_at_every_m1_edge(solver, m1):
    vs, ds = JC.s_grids(m1, 3)
    mu, sig = JC.laws_for(3)
    isolate(solver, "m1 edge", m1, JC.M1_M2, vs, ds, mu, sig, seed=m1)


@pytest.mark.parametrize("m2", JC.M2_EDGES)
def test_substep_at_every_m2_edge(solver, m2):
    vs, ds = JC.s_grids(JC.M2_M1, 3)
    mu, sig = JC.laws_for(3, first=1)
    isolate(solver, "m2 edge", JC.M2_M1, m2, vs, ds, mu, sig, seed=1000 + m2)


def test_substep_with_a_shared_matrix(solver):
    """300x12 x 40 on one grid and one dense law: several instances ride on one staged strip."""
    vs, ds = JC.s_grids(300, 40, same=True)
    isolate(solver, "shared", 300, 12, vs, ds, JC.DENSE[0][0], JC.DENSE[0][1], seed=77, shared=True)


@pytest.mark.parametrize("m1,m2", JC.ILL_SHAPES)
def test_substep_on_ill_conditioned_s_grids(solver, m1, m2):
    """One instance per placement of the tiny interval (R = 1e6).  The bound is the same: G_dev and P are the device's own."""
    places, _ = JC.ill_s_grids(m1)
    vs, ds = np.stack([p[1] for p in places]), np.stack([p[2] for p in places])
    assert Cm.interval_ratios(ds).min() >= 1e5
    mu, sig = JC.laws_for(len(places), pool=JC.ILL_LAWS)
    isolate(solver, "ill grids", m1, m2, vs, ds, mu, sig, seed=m1 + 3)


def test_the_rule_sees_one_entry_moved_by_1e_9(solver):
    """Reference-side self-test on the device's own P, U and G_dev at 300x12 and 1024x12: one entry of G_dev moved by 1e-9 of its row's
    max|G| before R is formed -- a near pair, a far pair, one in the last K tile that holds a node -- makes the check fail."""
    for m1 in (300, 1024):
        vs, ds = JC.s_grids(m1, 1)
        P, U, mats, avec = isolate(solver, "teeth", m1, 12, vs, ds, np.array([JC.DENSE[0][0]]), np.array([JC.DENSE[0][1]]), seed=5)
        for name, (i, l) in JC.teeth_positions(m1).items():
            r, at = JC.substep_ratio(P[0], U[0], mats[0], avec[0], m1, 12, perturb=(i, l, 1e-9))
            print("m1 = %d, %s (%d, %d): %.1f of the bound at %s" % (m1, name, i, l, r, at))
            assert r > 1.0 and at[1] == i, (name, r, at)


# ---- item 2: the matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1", JC.M1_EDGES)
def test_matrix_on_well_conditioned_grids_at_every_edge(solver, m1):
    """All rows against the numpy generator at the entry bound, every law of the table."""
    K = Cm.well_conditioned_strikes(m1, 1)[0]
    g = H.GridViewsBatch.for_strikes(m1, 8, Cm.S_0, Cm.V_0, [K])
    vs = g.Vec_s[0]
    assert Cm.interval_ratios(g.Delta_s)[0] <= Cm.COND_MAX
    for mu, sig in JC.LAWS:
        G, Gr = solver.debug_jump_matrix(vs, mu, sig), JR.generator(vs, mu, sig)
        worst = (np.abs(G - Gr) / JC.entry_bound(vs, mu, sig)[:, None]).max()
        print("m1 = %d (%g, %g): worst entry at %.3f of its bound" % (m1, mu, sig, worst))
        assert np.isfinite(G).all() and worst <= 1.0 and not G[0].any()
        assert JC.row_sums_ratio(G, vs) <= 1.0  # |G 1|, |G s| <= 1e-12 max s


@pytest.mark.parametrize("m1,m2", JC.ILL_SHAPES)
def test_matrix_on_ill_conditioned_s_grids(solver, m1, m2):
    places, K = JC.ill_s_grids(m1)
    fix = json.load(open(os.path.join(HERE, "golden", JC.ILL_FIXTURE)))["cases"]
    worst = np.zeros(4)
    for name, vs, ds, tiny in places:
        for law in JC.ILL_LAWS:
            rec = fix[JC.ill_key(m1, name, law)]
            assert rec["rows"] == JC.ill_rows(m1, tiny) and rec["tiny"] == tiny
            worst = np.maximum(worst, JC.ill_matrix_check("m1 = %d, %s" % (m1, name), solver.debug_jump_matrix(vs, *law), vs, K, tiny, law, rec))
    print("m1 = %d: worst margins %s" % (m1, worst))
    assert (worst <= 1.0).all(), worst


# ---- item 3: launches that do not start at instance 0 ---------------------------------------------------------------------------------------
def test_two_streams_cut_a_bates_batch_in_two_launches(solver):
    """50x25 x5 with per-instance laws: the halves [0, 3) and [3, 5) on two streams give the bits of one launch and keep the
    reference's bound."""
    import test_gpu_jumps as T
    case = T.Case(50, 25, 5, 6, law=(np.array([0.5, 2.0, 0.3, 1.0, 0.7]), *JC.laws_for(5)))
    with tuned(solver, {"streams": 1}):
        U1, d1 = case.run(solver)
    with tuned(solver, {"streams": 2}):
        U2, d2 = case.run(solver)
    assert "two streams" not in d1 and "2 sub-batches" in d2 and "side by side on two streams" in d2 and d2.endswith(JUMP_WORDS), (d1, d2)
    assert np.array_equal(U1, U2)
    T.field_check("two streams", U2, case.ref())


@pytest.mark.parametrize("share", [0, 1])
def test_two_streams_cut_an_eight_column_jacobian_in_two_launches(solver, share):
    """50x25 x3: 27 instances as the halves 14 + 13, so the second launch starts inside a group (inst0 % n_src != 0)."""
    import test_gpu_jumps8 as T8
    case = T8.Case(50, 25, 3, 6)  # (the family's own per-instance laws: the bounds of its reference belong to them)
    out = {}
    for streams in (1, 2):
        with tuned(solver, {"streams": streams, "jump_share": share}):
            out[streams] = case.jac8(solver)
    (J1, b1, d1), (J2, b2, d2) = out[1], out[2]
    assert "two streams" not in d1 and "2 sub-batches of 14 13" in d2 and "side by side on two streams" in d2 and d2.endswith(T8.SEL_WORDS), (d1, d2)
    assert np.array_equal(J1, J2) and np.array_equal(b1, b2)
    T8.within_bounds("two streams, jump_share %d" % share, J2, b2, *case.ref())


# ---- item 4: wide laws over several steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2", [(50, 25), (300, 12)])
def test_wide_laws_over_four_steps(solver, m1, m2):
    """The dense laws against tests/jumps_ref.py at the family's 1e-10, N = 4.  The intensity keeps a |kbar| max(s_i / h_i) <= 1
    (asserted on the inputs): beyond it the explicit compensator amplifies round-off and the comparison means nothing."""
    import test_gpu_jumps as T
    n, N = 3, 4
    strikes, grids, _ = T.batch(m1, m2, n)
    mu, sig = JC.laws_for(n, pool=JC.DENSE)
    lam = np.array([JC.stable_intensity(grids.Vec_s[k], mu[k], sig[k], Cm.T / N) for k in range(n)])
    for k in range(n):
        assert lam[k] * (Cm.T / N) * abs(JR.kbar(mu[k], sig[k])) * JC.stiffness(grids.Vec_s[k]) <= 1.0
    case = T.Case(m1, m2, n, N, law=(lam, mu, sig))
    U, d = case.run(solver)
    assert d.endswith(JUMP_WORDS), d
    T.field_check("wide laws %dx%d" % (m1, m2), U, case.ref())
    with tuned(solver, STREAMING):
        P, _ = case.plain(solver)
    assert all(not np.array_equal(U[k], P[k]) for k in range(n))
