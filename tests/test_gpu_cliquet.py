"""Forward-start and cliquet sweeps on the device (hadi_cliquet_timestepping, hadi_compute_base_prices_cliquet,
hadi_compute_jacobian_cliquet): one case per kernel that applies the strike fixing -- the four whole-loop LDS kernels and
hadi_small_sch_kernel inside their time loop (hadi_fixing_lds), hadi_fixing_gather_kernel + hadi_fixing_kernel behind the streaming
kernels at every layout -- each with its tuning keys pinned and its kernel family asserted from describe_last_sweep().  The
reference is tests/cliquet_ref.py (oracle operators and line solves, the event in numpy); tests/test_cliquet_ref.py shows that a
reference node off by one, a shifted schedule, the other mode, a dropped fixing or a dropped weight moves it by >= 1e-4 of max|U|.
Every node of a v-row reads ONE node of the row and is then overwritten, the source node included: the placements below put that
node on every special slot of every layout.
Bounds (those of tests/test_gpu_barrier.py): field 1e-10 of the instance's max|U_ref| on well-conditioned grids (asserted),
prices 1e-9, J 2e-4."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import bermudan_ref as BR
import cliquet_ref as QR
import common as Cm
from fixing_cases import mixed_weights
from test_gpu_bermudan import LAYOUTS

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
SCHEMES = [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")]
DEFAULTS = {"small_grid": 1, "team_launch": -1, "resident_sweep": -1, "strip": -1, "pair_strips": -1, "small_seq": -1,
            "small_pairs": -1, "small_sch": -1, "small_waves": 0, "streams": 0, "graph": 1}
STREAMING = {"small_grid": 0, "team_launch": 0, "resident_sweep": 0}
FIX_LOOP, FIX_STREAM = "cliquet: strike fixing at the end of", "cliquet: hadi_fixing_kernel after each of"
INVALID, UNSUPPORTED, NOT_ON_GRID = 1, 2, 4  # enum hadi_status
SHARES, RETURN = H.FIX_SHARES, H.FIX_RETURN
# per-instance reference nodes (offsets from the node nearest the instance's strike) and modes, cycled through the batch
SHIFT, MODES = (0, 3, -2, 1, -5), (SHARES, RETURN, RETURN, SHARES, RETURN)


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


def st(**tuning):
    return {**STREAMING, **tuning}


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, put=False):
    """(strikes, grids, payoff) on well-conditioned grids, built once per shape and left unchanged."""
    strikes = Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = Cm.put_payoff(grids.Vec_s, strikes, m2) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0


class Case:
    def __init__(self, m1, m2, n, N, fix, div=False, put=False, scheme=0, theta=Cm.THETA, N_i=None, dt_i=None, i_ref=None, mode=None,
                 weights="mixed", payoff=None):
        self.m1, self.m2, self.n, self.N, self.fix, self.div, self.put, self.scheme, self.theta = m1, m2, n, N, fix, div, put, scheme, theta
        self.N_i, self.dt_i, self.payoff = N_i, dt_i, payoff
        self.strikes, self.grids, self.U0 = batch(m1, m2, n, put)
        self.dt = Cm.T / N
        vs = self.grids.Vec_s
        if i_ref is None:
            i_ref = [int(np.argmin(np.abs(vs[k] - self.strikes[k]))) + SHIFT[k % 5] for k in range(n)]
        self.i_ref = list(i_ref)
        self.ref_spot = np.array([vs[k][self.i_ref[k]] for k in range(n)])
        self.mode = [MODES[k % 5] for k in range(n)] if mode is None else list(mode)
        self.weights = (mixed_weights(fix) if fix is not None else None) if isinstance(weights, str) else weights

    def kw(self):
        k = dict(variant=H.DIV if self.div else H.EU, dividends=H.Dividends(*Cm.DIVS) if self.div else None, scheme=self.scheme)
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.N_i is not None:
            k["per_instance"] = {"N_i": self.N_i, "delta_t_i": self.dt_i}
        if self.payoff is not None:
            k["U_0"] = self.payoff
        return k

    def head(self):
        return (self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F) + MODEL + (self.grids,)

    def fw(self, fix, weights):
        fix = self.fix if fix is None else fix
        return fix, (self.weights if weights == "own" else mixed_weights(fix) if weights == "mixed" else weights)

    def run(self, sv, fix=None, weights="own", ref_spot=None, mode=None, U=None, **over):
        U = self.U0.copy() if U is None else U
        fix, w = self.fw(fix, weights)
        sv.cliquet_timestepping(*self.head(), U, fix, self.ref_spot if ref_spot is None else ref_spot, self.mode if mode is None else mode,
                                w, **{**self.kw(), **over})
        return U, sv.describe_last_sweep()

    def ref(self, fix=None, weights="own", rows=None, ref_spot=None, mode=None):
        g = self.grids
        fix, w = self.fw(fix, weights)
        return QR.solve_batch(self.m1, self.m2, self.N, self.dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, g.Vec_s, g.Vec_v, g.Delta_s,
                              g.Delta_v, self.U0, fix, self.ref_spot if ref_spot is None else ref_spot,
                              np.asarray(self.mode if mode is None else mode), w, self.payoff, dividends=Cm.DIVS if self.div else None,
                              put_strikes=self.strikes if self.put else None, scheme=self.scheme, N_i=self.N_i, dt_i=self.dt_i, rows=rows)


def field_check(name, U, Uo, rows=None):
    r = range(U.shape[0]) if rows is None else rows
    e = np.array([np.abs(U[k] - Uo[k]).max() / np.abs(Uo[k]).max() for k in r])
    print("%s: field error %.3e of max|U_ref|" % (name, e.max()))
    assert np.isfinite(e).all() and e.max() <= 1e-10, (name, e)


def check(sv, name, case, tuning, want, absent=(), rows=None):
    with tuned(sv, tuning):
        U, d = case.run(sv)
    for w in want:
        assert any(x in d for x in ((w,) if isinstance(w, str) else w)), (w, d)
    for a in absent:
        assert a not in d, (a, d)
    field_check(name, U, case.ref(rows=rows), rows)
    return U, d


# ---- the whole-loop LDS kernels, by tuning key, on 50x25 and 100x20 -----------------------------------------------------------
SMALL = [("block8", {"small_seq": 0, "small_waves": 8}, "hadi_small_kernel<%d,8,EU>"),
         ("block4", {"small_seq": 0, "small_waves": 4}, "hadi_small_kernel<%d,4,EU>"),
         ("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<%d>"),
         ("seq2", {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<%d>")]
PER3 = [[2, 5, 8], [5], [2, 8]]  # per-instance schedules over the steps [2, 5, 8]; the last date is the valuation date, n = N


@pytest.mark.parametrize("m1,m2,B", [(50, 25, 1), (100, 20, 2)], ids=["50x25", "100x20"])
@pytest.mark.parametrize("name,tuning,kernel", SMALL, ids=[s[0] for s in SMALL])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_whole_loop_kernels(solver, m1, m2, B, name, tuning, kernel, put):
    # (three instances: the pairs kernel's last block holds one)
    check(solver, "%s %dx%d" % (name, m1, m2), Case(m1, m2, 3, 8, [2, 5, 8], put=put), tuning, [kernel % B, FIX_LOOP + " 3 steps"],
          [FIX_STREAM])
    check(solver, "%s %dx%d per-instance" % (name, m1, m2), Case(m1, m2, 3, 8, PER3, put=put), tuning, [kernel % B, FIX_LOOP + " 3 steps"],
          [FIX_STREAM])


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("m1,m2,B", [(50, 25, 1), (100, 20, 2)], ids=["50x25", "100x20"])
def test_scheme_kernel(solver, scheme, theta, sname, m1, m2, B):
    check(solver, "small_sch %s %dx%d" % (sname, m1, m2), Case(m1, m2, 3, 6, [[1, 4, 6], [4], [1, 6]], scheme=scheme, theta=theta),
          {"small_sch": 1}, ["hadi_small_sch_kernel<%d,%s>" % (B, sname), FIX_LOOP], [FIX_STREAM])


# ---- hadi_fixing_gather_kernel + hadi_fixing_kernel at every layout of tests/test_gpu_bermudan.py -----------------------------
@pytest.mark.parametrize("name,m1,m2,N,tuning,want", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_fixing_kernel_layouts(solver, name, m1, m2, N, tuning, want):
    steps = sorted({max(1, N // 2), N})
    fix = [steps, steps[:1], steps[-1:]]
    check(solver, name, Case(m1, m2, 3, N, fix, put=True), tuning, want + [FIX_STREAM + " %d fixing steps" % len(steps)], [FIX_LOOP])


# ---- the reference node on every special slot of every layout -----------------------------------------------------------------
# one shape per (B, G): m1 = 40 (1, 1), 100 (2, 1), 200 (4, 1), 300 (8, 1), 600 (8, 2), 1100 (natural rows)
PLACEMENT_SHAPES = [(40, 1, 1), (100, 2, 1), (200, 4, 1), (300, 8, 1), (600, 8, 2), (1100, 1, 18)]


def placements(m1, B, G):
    """(i_ref, mode) of the batch: RETURN with i_ref = 0 (the special slot 64 B G) and m1; SHARES with 1 and m1; the last node of
    a lane and the first of the next; for two wavefronts per row the nodes 64 B and 64 B + 1 on either side of them; an odd and an
    even i_ref (the two halves of a 16-byte pair)."""
    out = [(0, RETURN), (m1, RETURN), (1, SHARES), (m1, SHARES), (2 * B, RETURN), (2 * B + 1, SHARES)]  # lane 1's last node, lane 2's first
    if G == 2:
        out += [(64 * B, SHARES), (64 * B + 1, RETURN)]
    odd = (m1 // 2) | 1
    return out + [(odd, RETURN), (odd + 1, SHARES)]


@pytest.mark.parametrize("m1,B,G", PLACEMENT_SHAPES, ids=["m1=%d" % s[0] for s in PLACEMENT_SHAPES])
def test_reference_node_placements_streaming(solver, m1, B, G):
    m2, N = 8, 2
    pl = placements(m1, B, G)
    case = Case(m1, m2, len(pl), N, [1, 2], put=True, i_ref=[p[0] for p in pl], mode=[p[1] for p in pl], weights=[0.5, 0.0])
    want = ["hadi_pass_a_seq<EU>"] if m1 > 1024 else ["hadi_pass_a<%d,%d," % (B, G), "hadi_pass_a_strip<%d," % B, "hadi_pass_a_pairs<"]
    check(solver, "placements m1=%d" % m1, case, st(), [tuple(want), FIX_STREAM])


@pytest.mark.parametrize("m1,B", [(40, 1), (100, 2)], ids=["m1=40", "m1=100"])
@pytest.mark.parametrize("name,tuning,kernel", SMALL, ids=[s[0] for s in SMALL])
def test_reference_node_placements_whole_loop(solver, m1, B, name, tuning, kernel):
    pl = placements(m1, B, 1)
    case = Case(m1, 8, len(pl), 2, [1, 2], put=True, i_ref=[p[0] for p in pl], mode=[p[1] for p in pl], weights=[0.5, 0.0])
    check(solver, "placements %s m1=%d" % (name, m1), case, tuning, [kernel % B, FIX_LOOP])


# ---- the exact-bit properties, in both paths ----------------------------------------------------------------------------------
EXACT_PATHS = [("block", {"small_seq": 0}, "hadi_small_kernel<"), ("seq", {"small_seq": 1, "small_pairs": 0}, "hadi_small_seq_kernel<"),
               ("seq2", {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"), ("streaming", st(), FIX_STREAM)]


@pytest.mark.parametrize("name,tuning,want", EXACT_PATHS, ids=[p[0] for p in EXACT_PATHS])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_exact_bits_with_zero_weights(solver, name, tuning, want, m1, m2):
    """One fixing at the last step, no weights: SHARES leaves node (i_ref, j) with the bits of the run without the fixing; RETURN
    leaves every node of row j with them."""
    n, N = 4, 3
    case = Case(m1, m2, n, N, [N], put=True, mode=[SHARES, RETURN, SHARES, RETURN], weights=None)
    with tuned(solver, tuning):
        U, d = case.run(solver)
        assert want in d and "cliquet" in d, d
        V, _ = case.run(solver, fix=[], weights=None)
        W, _ = case.run(solver, weights=[0.0])  # an explicit weight of zero is no weight
    assert np.array_equal(U, W)
    Ur, Vr = U.reshape(n, m2 + 1, m1 + 1), V.reshape(n, m2 + 1, m1 + 1)
    for k in range(n):
        c = Vr[k][:, case.i_ref[k]]
        assert np.array_equal(Ur[k][:, case.i_ref[k]], c), k
        if case.mode[k] == RETURN:
            assert np.array_equal(Ur[k], np.repeat(c[:, None], m1 + 1, axis=1)), k
        else:
            assert not np.array_equal(Ur[k][:, case.i_ref[k] + 1], c), k
    field_check("exact bits " + name, U, case.ref())


# ---- identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{}, {"small_seq": 1, "small_pairs": 1}, st(), st(strip=1)], ids=["default", "seq2", "ring", "strips"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 30)], ids=["50x25", "100x30"])
def test_empty_schedule_is_DO_timestepping_bit_for_bit(solver, tuning, m1, m2):
    case = Case(m1, m2, 3, 5, [])
    with tuned(solver, tuning):
        U, d = case.run(solver)
        V = case.U0.copy()
        solver.DO_timestepping(*case.head(), V)
        d0 = solver.describe_last_sweep()
        assert d == d0 and "cliquet" not in d, d
        assert np.array_equal(U, V)
        W, d2 = case.run(solver, fix=[[], [], []], weights=None)  # a ragged schedule in which nobody has a date
        assert np.array_equal(W, V) and d2 == d
        _, d3 = case.run(solver, fix=[2, 4])
        assert d3.startswith(d0) and d3[len(d0):].startswith("; cliquet: "), (d0, d3)


# ---- schedules: every step, the valuation date, a dividend step, per-instance step grids ---------------------------------------
PER_INSTANCE = EXACT_PATHS


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
def test_fixing_on_every_step_and_at_the_valuation_date(solver, name, tuning, want):
    check(solver, "every step " + name, Case(50, 25, 3, 6, list(range(1, 7)), put=True), tuning, [want, "6 "])
    check(solver, "n = N " + name, Case(50, 25, 3, 6, [6], put=True), tuning, [want, "1 "])


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
def test_per_instance_schedules_with_rotated_step_grids(solver, name, tuning, want):
    """Five instances, each with its own (N_i, dt_i), reference node, mode, schedule and weights (one with none, one fixing at its
    own N_i): the pairs kernel holds instances of different N and different schedules in one wavefront."""
    N_i = [8, 5, 7, 3, 6]
    dt_i = [Cm.T / 8, 0.5 / 5, 0.8 / 7, 0.25 / 3, 0.6 / 6]
    fix = [[2, 8], [1, 3, 5], [], [3], [4]]
    check(solver, "per-instance " + name, Case(50, 25, 5, 8, fix, put=True, N_i=N_i, dt_i=dt_i), tuning, [want, "cliquet"])


def test_a_fixing_beyond_a_short_instances_N_is_refused(solver):
    case = Case(50, 25, 3, 6, [2, 5], put=True, N_i=[6, 4, 5], dt_i=[Cm.T / 6] * 3)
    with pytest.raises(H.HadiError) as e:
        case.run(solver)
    assert e.value.status == INVALID
    case.run(solver, fix=[2, 4])
    with pytest.raises(H.HadiError) as e:
        case.run(solver, fix=[[2, 6], [5], [1]])  # instance 1 has 4 steps
    assert e.value.status == INVALID


@pytest.mark.parametrize("name,tuning,want", PER_INSTANCE, ids=[p[0] for p in PER_INSTANCE])
@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_dividend_and_fixing_on_one_step(solver, name, tuning, want, put):
    """N = 20: the canonical dividends pay at the START of steps 4, 8, 11 and 16; the fixing acts at the END of 8 and 16."""
    assert BR.dividend_steps(20, Cm.T / 20, Cm.DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}
    check(solver, "dividend step " + name, Case(50, 25, 3, 20, [8, 16], div=True, put=put), tuning, [want, "cliquet"])


@pytest.mark.parametrize("scheme,theta,sname", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning,want", [("ring", 50, 25, st(small_sch=0), "hadi_pass_a"),
                                                     ("strips", 300, 80, st(small_sch=0, strip=1), "strip")], ids=["ring", "strips"])
def test_schemes_on_the_streaming_path(solver, scheme, theta, sname, path, m1, m2, tuning, want):
    check(solver, "%s %s" % (path, sname), Case(m1, m2, 2, 4, [2, 4], scheme=scheme, theta=theta), tuning, [want, sname, FIX_STREAM],
          ["hadi_small_sch_kernel"])


def test_a_payoff_that_is_not_the_initial_field(solver):
    """A capped cliquet: the initial condition and P are the local-return payoff; RETURN mode, weights 1, put boundary data."""
    m1, m2, n, N = 50, 25, 3, 8
    strikes, grids, _ = batch(m1, m2, n, True)
    for tuning, want in (({"small_seq": 0}, FIX_LOOP), (st(), FIX_STREAM)):
        case = Case(m1, m2, n, N, [2, 4, 6], put=True, mode=[RETURN] * n, weights=[1.0, 1.0, 1.0])
        pay = H.local_return_payoff(grids, case.ref_spot, 1.0, 0.0, 0.05)
        case.U0, case.payoff = pay, pay.copy()
        check(solver, "capped cliquet", case, tuning, [want])
        case.payoff = 2.0 * pay  # (U_0 is read, not the initial U)
        check(solver, "capped cliquet, P = 2 U", case, tuning, [want])


# ---- routing: never the team launch, never the resident sweep, sub-batches on two streams -------------------------------------
def test_team_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 140, 4, 3, [1, 3], put=True)
    with tuned(solver, {"team_launch": 1}):
        U, d = case.run(solver)
        assert "hadi_team_kernel" not in d and "row pass" in d and FIX_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:  # (eligibility itself: the plain call of the same batch takes the team)
            _, d0 = case.run(solver, fix=[], weights=None)
            assert "hadi_team_kernel" in d0 and "cliquet" not in d0, d0
    field_check("team-eligible", U, case.ref(rows=[0, 3]), [0, 3])


def test_resident_eligible_batch_runs_the_streaming_kernels(solver):
    case = Case(300, 80, 256, 2, [1, 2])
    with tuned(solver, {"resident_sweep": 1, "strip": 1}):
        U, d = case.run(solver)
        assert "hadi_sweep_resident" not in d and "hadi_pass_a_strip<8,EU>" in d and FIX_STREAM in d, d
        if solver.device_info()["compute_units"] == 256:
            _, d0 = case.run(solver, fix=[], weights=None)
            assert "hadi_sweep_resident" in d0 and "cliquet" not in d0, d0
    rows = [0, 100, 255]
    field_check("resident-eligible", U, case.ref(rows=rows), rows)


def test_sub_batches_on_two_streams(solver):
    """512x256 x 320 = a round of 256 and a remainder of 64: each sub-batch launches the two fixing kernels on its own stream, with
    its own offset into U, the payoff, the tables and c (per-instance rows: odd instances fix at step 2, even ones never)."""
    n, N = 320, 3
    fix = [[2] if k % 2 else [] for k in range(n)]
    case = Case(512, 256, n, N, fix, put=True, weights=[[0.5] if k % 2 else [] for k in range(n)])
    U, d = case.run(solver)
    assert "sub-batches" in d and "two streams" in d and FIX_STREAM in d, d
    rows = [0, 255, 256, 319]
    Uo = case.ref(rows=rows)
    field_check("two streams", U, Uo, rows)
    plain = case.ref(fix=[[] for _ in range(n)], weights=None, rows=[255])
    assert np.abs(Uo[255] - plain[255]).max() / np.abs(Uo[255]).max() >= 1e-4  # (the schedule matters at this N)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def test_device_memory_inputs(solver):
    import torch
    case = Case(50, 25, 3, 6, [2, 6], put=True)
    dev = torch.device("cuda", 0)
    for tuning in ({"small_seq": 0}, st()):
        with tuned(solver, tuning):
            host, _ = case.run(solver)
            U = torch.from_numpy(case.U0.copy()).to(dev)
            solver.cliquet_timestepping(*case.head()[:-1], case.grids.to(dev), U, case.fix, case.ref_spot, case.mode, case.weights, **case.kw())
            assert np.array_equal(U.cpu().numpy(), host)
    field_check("device memory", host, case.ref())


# ---- the launchers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,tuning,want", [(50, 25, {"small_seq": 1, "small_pairs": 1}, "hadi_small_seq2_kernel<"),
                                               (50, 25, st(), FIX_STREAM), (128, 64, st(), FIX_STREAM)],
                         ids=["50x25-lds", "50x25-streaming", "128x64-streaming"])
def test_launchers(solver, m1, m2, tuning, want):
    n, N, eps = 3, 6, 1e-6
    strikes, grids, U0 = batch(m1, m2, n, True)
    fix = [[2, 6], [3], [1, 4, 6]]
    wts = [[1.0, 0.0], [0.5], [0.0, 0.25, 1.0]]
    vs = grids.Vec_s
    # the price is read at S_0: instance 0 fixes there, the others at nodes of their own
    i_ref = [QR.find_node(vs[0], Cm.S_0), int(np.argmin(np.abs(vs[1] - strikes[1]))) + 3, int(np.argmin(np.abs(vs[2] - strikes[2]))) - 2]
    ref = np.array([vs[k][i_ref[k]] for k in range(n)])
    mode = [SHARES, RETURN, SHARES]
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s, "option_type": H.PUT, "strikes": strikes}
    size = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, size)
    ws.U[...] = U0
    refkw = dict(put_strikes=strikes, V_0_i=v0s, ref_spot=ref, mode=np.asarray(mode), weights=wts)
    args = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F) + MODEL + (Cm.S_0, Cm.V_0, grids.Vec_s, grids.Delta_s, U0, fix)
    with tuned(solver, tuning):
        prices = solver.compute_base_prices_cliquet(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                    grids, ws, fix, ref, mode, wts, per_instance=per)
        assert want in solver.describe_last_sweep() and "cliquet" in solver.describe_last_sweep()
        J, base = solver.compute_jacobian_cliquet(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, size, N, Cm.THETA, Cm.T / N, n,
                                                  grids, U0.copy(), fix, ref, mode, wts, eps=eps, per_instance=per)
        assert want in solver.describe_last_sweep() and "cliquet" in solver.describe_last_sweep()
    po, Fo = QR.base_prices(*args, **refkw)
    Jo, bo = QR.jacobian(*args, eps=eps, **refkw)
    print("launchers %dx%d: prices %.2e, J %.2e" % (m1, m2, np.abs(prices - po).max(), np.abs(J - Jo).max()))
    field_check("launcher field", ws.U, Fo)
    assert np.abs(prices - po).max() <= 1e-9 and np.abs(base - bo).max() <= 1e-9
    assert np.array_equal(base, prices)
    assert np.abs(J - Jo).max() <= 2e-4


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(solver):
    case = Case(50, 25, 3, 6, [2, 6])
    ct, head, U0 = solver.cliquet_timestepping, case.head(), case.U0
    ref, mode = case.ref_spot, case.mode
    for bad in ([0, 3], [3, 3], [4, 2], [7], [-1], [2, 0, 4], [[2], [7], [1]], [[2, 4], [4, 2], [1]]):
        assert status(ct, *head, U0.copy(), bad, ref, mode) == INVALID, bad
    # the reference spots, the modes and the weights
    nan3, inf3 = np.array([np.nan, 1.0, 1.0]), np.array([1.0, np.inf, 1.0])
    assert status(ct, *head, U0.copy(), [2], ref * nan3, mode) == INVALID
    assert status(ct, *head, U0.copy(), [2], ref * inf3, mode) == INVALID
    assert status(ct, *head, U0.copy(), [2], ref, [0, 2, 1]) == INVALID
    assert status(ct, *head, U0.copy(), [2], ref, [0, -1, 1]) == INVALID
    assert status(ct, *head, U0.copy(), [2, 4], ref, mode, [1.0, np.nan]) == INVALID
    assert status(ct, *head, U0.copy(), [2, 4], ref, mode, [np.inf, 0.0]) == INVALID
    ct(*head, U0.copy(), [[2, 4], [3], [1]], ref, mode, [[1.0, 0.0], [1.0], [0.5]])  # (a ragged weight list is padded as the schedule is)
    zero = np.array([0.0, ref[1], ref[2]])
    assert status(ct, *head, U0.copy(), [2], zero, SHARES) == INVALID                  # SHARES at node 0: the grid's 0
    ct(*head, U0.copy(), [2], zero, [RETURN, SHARES, SHARES])                          # ... RETURN there is fine
    assert status(ct, *head, U0.copy(), [2], [1e-10, ref[1], ref[2]], SHARES) == INVALID
    # a reference spot between two nodes: off the grid
    vs = case.grids.Vec_s
    off = np.array([ref[0], 0.5 * (vs[1][20] + vs[1][21]), ref[2]])
    for tuning in ({"small_seq": 0}, {"small_seq": 1, "small_pairs": 1}, st()):
        with tuned(solver, tuning):
            assert status(ct, *head, U0.copy(), [2], off, mode) == NOT_ON_GRID
    for variant in (H.AM, H.AM_DIV):
        assert status(ct, *head, U0.copy(), [2], ref, mode, variant=variant, dividends=H.Dividends(*Cm.DIVS)) == UNSUPPORTED
    # what check_problem refuses keeps its status: a scheme with dividends
    assert status(ct, *head, U0.copy(), [2], ref, mode, variant=H.DIV, dividends=H.Dividends(*Cm.DIVS), scheme=H.SCHEME_MCS) == UNSUPPORTED
    # the raw ABI: a NULL struct, fix_rows, n_fix < 0, NULL steps, NULL ref_spot_i, the fp32 state, NULL outputs
    lib, h = solver._lib, solver._h
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())

    def cliquet(n_fix, steps, rows, with_ref=True):
        q, keep = solver._cliquet(3, [], ref, mode, None)
        arr = None if steps is None else np.asarray(steps, dtype=np.int32)
        q.n_fix, q.fix_rows = n_fix, rows
        q.fix_steps = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int))
        if not with_ref:
            q.ref_spot_i = None
        return q, (keep, arr)

    assert lib.hadi_cliquet_timestepping(h, C.byref(p), None) == INVALID
    for n_fix, steps, rows in ((2, [2, 6, 2, 6], 2), (2, [2, 6], 0), (-1, [2, 6], 1), (2, None, 1)):
        q, keep = cliquet(n_fix, steps, rows)
        assert lib.hadi_cliquet_timestepping(h, C.byref(p), C.byref(q)) == INVALID, (n_fix, steps, rows)
    q, keep = cliquet(2, [2, 6], 1, with_ref=False)
    assert lib.hadi_cliquet_timestepping(h, C.byref(p), C.byref(q)) == INVALID
    good, keep = cliquet(2, [2, 6], 1)
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_cliquet_timestepping(h, C.byref(p32), C.byref(good)) == UNSUPPORTED
    pv = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_base_prices_cliquet(h, C.byref(pv), Cm.S_0, Cm.V_0, C.byref(good), None) == INVALID
    out = np.zeros(3)
    assert lib.hadi_compute_base_prices_cliquet(h, C.byref(pv), Cm.S_0, Cm.V_0, None, C.c_void_p(out.ctypes.data)) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_jacobian_cliquet(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, C.byref(good), None, C.c_void_p(out.ctypes.data)) == INVALID
    assert lib.hadi_compute_jacobian_cliquet(h, C.byref(pj), Cm.S_0, Cm.V_0, 1e-6, None, None, None) == INVALID
    # and the handle still works
    assert lib.hadi_cliquet_timestepping(h, C.byref(p), C.byref(good)) == 0
    field_check("after the refusals", case.run(solver)[0], case.ref())


def test_helpers_fixing_steps_and_local_return_payoff():
    assert H.fixing_steps(1.0, 0.05, [0.0, 0.25, 0.5, 0.75]) == [5, 10, 15, 20]
    for bad in ([0.26], [1.0], [-0.05], [0.25, 0.25]):
        with pytest.raises(ValueError):
            H.fixing_steps(1.0, 0.05, bad)
    strikes, grids, _ = batch(50, 25, 3, True)
    vs = grids.Vec_s
    ref = np.array([vs[0][20], vs[1][25], vs[2][30]])
    P = H.local_return_payoff(grids, ref, 1.0, 0.0, [0.05, 0.08, 0.1]).reshape(3, 26, 51)
    for k in range(3):
        want = np.minimum(np.maximum(vs[k] / ref[k] - 1.0, 0.0), [0.05, 0.08, 0.1][k])
        assert np.array_equal(P[k], np.repeat(want[None, :], 26, axis=0))
    assert P[0][3, 20] == 0.0 and P[0][3, 50] == 0.05
    Q = H.local_return_payoff(grids, 100.0, strike=0.9).reshape(3, 26, 51)
    assert np.array_equal(Q[1][7], vs[1] / 100.0 - 0.9)


# ---- the recorded routes ------------------------------------------------------------------------------------------------------
def test_recorded_routes(solver):
    """tests/golden/route_selection_cliquet.json (tools/record_cliquet_routes.py): the device words every recorded call as it did."""
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import record_cliquet_routes as R
    fix = json.load(open(R.FIXTURE))
    assert [c[0] for c in R.CASES] == [r["name"] for r in fix["cases"]]
    same_device = solver.device_info()["compute_units"] == fix["cu_count"]  # (the cut of a batch depends on the number of CUs)
    for case, row in zip(R.CASES, fix["cases"]):
        if not same_device and case[1] > 8:
            continue
        d0, d1 = R.describe(solver, H, np, case)
        assert (d0, d1) == (row["plain"], row["cliquet"]), (case[0], d0, d1)


# ---- graph cache --------------------------------------------------------------------------------------------------------------
def test_graph_cache(solver):
    """The same call twice replays; a call with other reference nodes, modes and weights but the same schedule replays too -- the
    tables and the located nodes are data, uploaded again whatever the cache holds -- and is right; another schedule captures anew."""
    case = Case(50, 25, 3, 7, [3, 7], put=True)  # (seven steps: no other test of the session has captured this loop)
    A, B = [3, 7], [4, 7]
    UA, UB = case.ref(fix=A), case.ref(fix=B)
    assert np.abs(UA - UB).max() / np.abs(UA).max() >= 1e-4
    vs = case.grids.Vec_s
    other_ref = np.array([vs[k][case.i_ref[k] + 4] for k in range(3)])
    other_mode, other_w = [RETURN, SHARES, SHARES], [0.75, 0.5]
    UC = case.ref(fix=A, ref_spot=other_ref, mode=other_mode, weights=other_w)
    assert np.abs(UA - UC).max() / np.abs(UA).max() >= 1e-4
    with tuned(solver, st(graph=1)):
        case.run(solver, fix=[1, 2, 5])  # (the buffers this shape needs are grown: growing one would empty the cache)
        c0 = Cm.graph_counts(solver)
        first = case.run(solver, fix=A)
        c1 = Cm.graph_counts(solver)
        again = case.run(solver, fix=A)
        c2 = Cm.graph_counts(solver)
        C_, dC = case.run(solver, fix=A, ref_spot=other_ref, mode=other_mode, weights=other_w)
        c3 = Cm.graph_counts(solver)
        second = case.run(solver, fix=B)
        c4 = Cm.graph_counts(solver)
    assert all(FIX_STREAM in d for _, d in (first, again, second)) and FIX_STREAM in dC
    d1, d2, d3, d4 = (Cm.graph_delta(a, b) for a, b in ((c0, c1), (c1, c2), (c2, c3), (c3, c4)))
    assert (d1["captures"], d1["replays"]) == (1, 0), d1
    assert (d2["captures"], d2["replays"]) == (0, 1), d2
    assert (d3["captures"], d3["replays"]) == (0, 1), d3
    assert (d4["captures"], d4["replays"]) == (1, 0), d4
    field_check("A", first[0], UA)
    assert np.array_equal(first[0], again[0])
    field_check("A with other nodes, modes and weights", C_, UC)
    field_check("B", second[0], UB)
