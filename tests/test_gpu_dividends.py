"""Dividend schedules beyond the one fixture, on every implementation of the jump and through the time loop of hadi_api.hip
(the union of paying steps in the graph key, materialise / dematerialise around the jump for the American P representation,
widen / narrow for the fp32 state, the per-sub-batch offset into the flag table).

Every case compares the full field (and lambda_bar for American variants) with the oracle run with the same schedule -- the
oracle restates the reference's dating loop and linear scan on its own --, at the suite's bounds: field 1e-10 max|U_oracle|,
lambda_bar 1e-8 max(1, max|lambda|), fp32 state 2e-7 N.  Every case asserts through describe_last_sweep() that the kernel it
is named for ran, and through tests/dividend_schedules.py -- on the host, from the inputs alone -- that its schedule reaches
the branch it is named for on the grid it uses.  All grids obey the 30x conditioning rule and assert it.

Two things the schedules showed about the dating rule itself (both are the reference's behaviour, mirrored by the library and by
the oracle): two paying steps are never adjacent, so `every_step` and `on_grid` (a date in every step's interval) pay on step 1
only -- `alternate` and `on_grid_odd` are the densest schedules that are paid in full; and with N = 10 the fixture's date 0.6 is
dropped (the index reaches it on step 6, and 6 * 0.1 = 0.6000000000000001 > 0.6)."""
import contextlib
import functools
import random

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm
import dividend_schedules as D
import greeks_ref as G

pytestmark = pytest.mark.gpu

R_F = 0.01
FIELD_RTOL = 1e-10
DEFAULTS = {"small_grid": 1, "graph": 1, "small_seq": -1, "small_pairs": -1, "small_waves": 0, "strip": -1, "team_launch": -1,
            "american_p": 1, "streams": 0, "pair_strips": -1}
OV = {H.DIV: O.DIV, H.AM_DIV: O.AM_DIV, H.EU: O.EU, H.AM: O.AM}


@pytest.fixture(scope="module")
def h():
    """A handle of this module's own: every case sets tuning keys, none leaks into the session's handle."""
    s = H.HestonADI(0)
    yield s
    s.close()


@contextlib.contextmanager
def tuned(h, tune):
    for k, v in tune.items():
        h.set_tuning(k, v)
    try:
        yield
    finally:
        for k in tune:
            h.set_tuning(k, DEFAULTS[k])


def _has(d, present, absent=()):
    for e in present:
        assert e in d, (e, d)
    for e in absent:
        assert e not in d, (e, d)


# ---- inputs and the oracle's answers, computed once and shared ----------------------------------------------------------------
def _s_axis(kind, m1):
    if kind == "uniform":
        return np.linspace(10.0, 400.0, m1 + 1)
    assert kind == "geometric"
    return 10.0 * 40.0 ** (np.arange(m1 + 1) / m1)


@functools.lru_cache(maxsize=None)
def _inputs(m1, m2, n, put=False, kind="sinh"):
    """(strikes, grids, U_0): n well-conditioned strikes; kind "uniform" / "geometric" overwrites the s-axis of every instance
    with a caller grid on [10, 400] that does not start at 0."""
    strikes = Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), strikes)
    if kind != "sinh":
        s = _s_axis(kind, m1)
        grids.Vec_s = np.ascontiguousarray(np.tile(s, (n, 1)))
        grids.Delta_s = np.ascontiguousarray(np.tile(np.diff(s), (n, 1)))
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    return strikes, grids, U0


def _key(sch):
    return tuple(tuple(float(x) for x in a) for a in sch)


@functools.lru_cache(maxsize=None)
def _oracle_one(m1, m2, n, k, N, dt, variant, put, sch, fp32=False, kind="sinh"):
    """Instance k of the batch through the oracle: (U_T, lambda_bar_T or None); sch as _key() makes it."""
    strikes, grids, U0 = _inputs(m1, m2, n, put, kind)
    p = O.make_params(m1, m2, N, dt, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, OV[variant],
                      sch if variant in (H.DIV, H.AM_DIV) else None, state_fp32=1 if fp32 else 0,
                      option_type=O.PUT if put else O.CALL, strikes=[strikes[k]] if put else None)
    U, lam, _ = O.solve(p, grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k], U0[k], U0[k])
    assert np.isfinite(U).all()
    return U, lam


def _oracle(m1, m2, n, Ns, dts, variant, put, sch, fp32=False, kind="sinh"):
    r = [_oracle_one(m1, m2, n, k, int(Ns[k]), float(dts[k]), variant, put, _key(sch), fp32, kind) for k in range(n)]
    return np.stack([u for u, _ in r]), (np.stack([l for _, l in r]) if r[0][1] is not None else None)


def _solve(h, m1, m2, n, N, variant, put, sch, fp32=False, kind="sinh", per=None, T=Cm.T):
    strikes, grids, U0 = _inputs(m1, m2, n, put, kind)
    american = variant in (H.AM, H.AM_DIV)
    U = U0.copy()
    lam = np.zeros_like(U0) if american else None
    h.DO_timestepping(m1, m2, N, T / N, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U, variant=variant,
                      U_0=U0 if american else None, lambda_bar=lam,
                      dividends=H.Dividends(*sch) if variant in (H.DIV, H.AM_DIV) else None, per_instance=per,
                      state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64, option_type=H.PUT if put else H.CALL,
                      strikes=strikes if put else None)
    return U, lam, h.describe_last_sweep()


def _check(U, lam, Uo, lamo, label, rtol=FIELD_RTOL):
    scale = np.abs(Uo).max()
    err = np.abs(U - Uo).max()
    print("%s: field error %.3e, max|U_oracle| %.3e, ratio %.3e" % (label, err, scale, err / scale if scale else 0.0))
    assert np.isfinite(U).all(), label
    assert err <= rtol * scale, "%s: field error %.3e (scale %.3e, bound %.1e)" % (label, err, scale, rtol)
    if lamo is not None:
        lerr, lscale = np.abs(lam - lamo).max(), max(1.0, np.abs(lamo).max())
        print("%s: lambda_bar error %.3e, scale %.3e" % (label, lerr, lscale))
        assert lerr <= 1e-8 * lscale, "%s: lambda_bar error %.3e (scale %.3e)" % (label, lerr, lscale)


def _require(name, N, dt, sch, m1, m2, n, put=False, kind="sinh"):
    _, grids, _ = _inputs(m1, m2, n, put, kind)
    return [D.requirement(name, N, dt, sch, grids.Vec_s[k]) for k in range(n)]


# ---- the execution paths --------------------------------------------------------------------------------------------------
# route: shape, batch, steps, tuning, the variants it admits, and what describe_last_sweep() must (not) say, by "american"
def _route(m1, m2, n, N, tune, european=None, american=None, absent=(), fp32=False):
    return dict(m1=m1, m2=m2, n=n, N=N, tune=tune, kernel={False: european, True: american}, absent=absent, fp32=fp32)


ROUTES = {
    "small4": _route(50, 25, 3, 20, {"small_waves": 4, "small_seq": 0}, ["hadi_small_kernel<1,4,EU>"], ["hadi_small_kernel<1,4,AM>"]),
    "small8": _route(50, 25, 3, 20, {"small_waves": 8, "small_seq": 0}, ["hadi_small_kernel<1,8,EU>"], ["hadi_small_kernel<1,8,AM>"]),
    "seq": _route(50, 25, 3, 20, {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<1>"]),
    "seq2_odd_batch": _route(50, 25, 3, 20, {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<1>"]),
    "stream1_pair": _route(50, 25, 3, 20, {"small_grid": 0, "american_p": 0}, ["hadi_pass_a<1,1,"], ["hadi_pass_a<1,1,"], absent=["AM-P"]),
    "stream1_P": _route(50, 25, 3, 20, {"small_grid": 0}, ["hadi_pass_a<1,1,"], ["hadi_pass_a<1,1,", "AM-P"]),
    "stream2": _route(128, 64, 2, 10, {"team_launch": 0}, ["hadi_pass_a<2,1,"], ["hadi_pass_a<2,1,", "AM-P"]),
    "strips8": _route(300, 80, 2, 10, {"strip": 1, "team_launch": 0}, ["hadi_pass_a_strip<8,EU>"], ["hadi_pass_a_strip<8,AM-P>"]),
    "paired_strips": _route(600, 40, 2, 10, {"strip": 1}, ["hadi_pass_a_strip<8,EU,double,2>"], ["hadi_pass_a_strip<8,AM-P,double,2>"]),
    "fp32_300x80": _route(300, 80, 2, 10, {"strip": 1, "team_launch": 0}, ["hadi_pass_a_strip<8,EU,float>", "fp32 state"], fp32=True),
    "fp32_50x25": _route(50, 25, 3, 20, {"small_grid": 0}, ["hadi_pass_a<1,1,", "float"], fp32=True),
    "team4": _route(150, 60, 3, 10, {"team_launch": 1}, ["hadi_team_kernel<4>"]),
    "team8": _route(300, 80, 3, 10, {"team_launch": 1}, ["hadi_team_kernel<8>"]),
    "seq_passes": _route(1030, 20, 1, 3, {}, ["hadi_pass_a_seq<EU>", "hadi_pass_b"], ["hadi_pass_a_seq<AM>"]),
}

# the path matrix: (route, variant, put); every row takes every named schedule (the sequential passes: the four that 3 steps reach)
MATRIX = [(r, v, put) for r in ("small4", "small8") for v in (H.DIV, H.AM_DIV) for put in (False, True)] + [
    ("seq", H.DIV, False), ("seq", H.DIV, True), ("seq2_odd_batch", H.DIV, False),
    ("stream1_pair", H.AM_DIV, False), ("stream1_P", H.AM_DIV, False), ("stream2", H.DIV, False),
    ("strips8", H.DIV, False), ("strips8", H.AM_DIV, False), ("paired_strips", H.AM_DIV, True),
    ("fp32_300x80", H.DIV, False), ("fp32_50x25", H.DIV, False),
    ("team4", H.DIV, False), ("team4", H.DIV, True), ("team8", H.DIV, False), ("team8", H.DIV, True)]
VNAME = {H.DIV: "DIV", H.AM_DIV: "AM_DIV"}


def _row_id(row):
    return "%s-%s-%s" % (row[0], VNAME[row[1]], "put" if row[2] else "call")


def _run_route(h, route, variant, put, name, sch, N=None, label=None):
    r = ROUTES[route]
    m1, m2, n, N = r["m1"], r["m2"], r["n"], r["N"] if N is None else N
    american = variant == H.AM_DIV
    assert r["kernel"][american] is not None, "route %s does not take %s" % (route, VNAME[variant])
    if name is not None:
        _require(name, N, Cm.T / N, sch, m1, m2, n, put)
    with tuned(h, r["tune"]):
        U, lam, d = _solve(h, m1, m2, n, N, variant, put, sch, fp32=r["fp32"])
    _has(d, r["kernel"][american], r["absent"])
    Uo, lamo = _oracle(m1, m2, n, [N] * n, [Cm.T / N] * n, variant, put, sch, fp32=r["fp32"])
    _check(U, lam, Uo, lamo, label or "%s %s %s %s" % (route, VNAME[variant], "put" if put else "call", name),
           rtol=2e-7 * N if r["fp32"] else FIELD_RTOL)
    return U, lam


@pytest.mark.parametrize("name", D.NAMES)
@pytest.mark.parametrize("row", MATRIX, ids=_row_id)
def test_named_schedules_on_every_path(h, row, name):
    route, variant, put = row
    N = ROUTES[route]["N"]
    _run_route(h, route, variant, put, name, D.named(N, Cm.T / N, Cm.T)[name])


@pytest.mark.parametrize("name", ["step1", "big_cash", "same_step", "zero"])
def test_named_schedules_on_the_sequential_passes(h, name):
    """1030x20: more than 1024 s-intervals, natural order of the sequential row pass; three steps, so the four schedules that
    reach their branch within three steps."""
    _run_route(h, "seq_passes", H.AM_DIV, False, name, D.named(3, Cm.T / 3, Cm.T)[name])


@pytest.mark.parametrize("name", D.NAMES)
def test_graph_replay_equals_the_plain_stream(h, name):
    """150x60 on the streaming kernels: the captured time loop (the union of paying steps decides where it has a jump node) and
    the same launches on the plain stream give bit-identical fields, within bound of the oracle."""
    m1, m2, n, N = 150, 60, 2, 10
    sch = D.named(N, Cm.T / N, Cm.T)[name]
    _require(name, N, Cm.T / N, sch, m1, m2, n)
    out = {}
    for graph in (1, 0):
        with tuned(h, {"graph": graph, "team_launch": 0}):
            g0 = Cm.graph_counts(h)
            U, _, d = _solve(h, m1, m2, n, N, H.DIV, False, sch)
            dg = Cm.graph_delta(g0, Cm.graph_counts(h))
        _has(d, ["hadi_pass_a<4,1,"], ["hadi_team_kernel"])
        assert dg["captures"] + dg["replays"] == graph, (graph, dg)
        out[graph] = U
    assert np.array_equal(out[1], out[0])
    Uo, _ = _oracle(m1, m2, n, [N] * n, [Cm.T / N] * n, H.DIV, False, sch)
    _check(out[1], None, Uo, None, "graph 150x60 DIV %s" % name)


# ---- per-instance step grids x schedules ------------------------------------------------------------------------------------
PER_T = [0.5, 1.0, 1.5, 0.25, 0.7]  # (the (T, N) of test_dividends_with_per_instance_maturities)
PER_N = [10, 20, 30, 20, 23]
PER_SCHEDULES = ["cluster", "same_step", "on_grid", "beyondT"] + ["random%d" % k for k in range(8)]


def _per_schedule(name):
    """Named ones laid out for instance 1's step grid (N = 20, dt = 0.05); random ones from their own seed."""
    if name.startswith("random"):
        return D.random_schedule(random.Random(7000 + int(name[6:])), 20, 0.05)
    return D.named(20, 0.05, 1.0)[name]


@pytest.mark.parametrize("name", PER_SCHEDULES)
@pytest.mark.parametrize("path,m1,m2,variant,tune,kernel", [
    ("small", 50, 25, H.AM_DIV, {}, "hadi_small_kernel<1,"),
    ("streaming", 50, 25, H.AM_DIV, {"small_grid": 0}, "hadi_pass_a<1,1,"),
    ("team", 150, 60, H.DIV, {"team_launch": 1}, "hadi_team_kernel<4>")], ids=["small", "streaming", "team"])
def test_per_instance_step_grids(h, path, m1, m2, variant, tune, kernel, name):
    """Every instance dates the shared schedule on ITS OWN step grid (its row of the flag table); each against its own oracle
    solve."""
    n = len(PER_T)
    sch = _per_schedule(name)
    dts = [t / k for t, k in zip(PER_T, PER_N)]
    paid = [D.paying_steps(PER_N[k], dts[k], sch[0]) for k in range(n)]
    assert len({tuple(sorted(p)) for p in paid if p}) >= 2, paid  # at least two instances pay, on different steps
    if not name.startswith("random"):
        _require(name, 20, 0.05, sch, m1, m2, n)
    with tuned(h, tune):
        U, lam, d = _solve(h, m1, m2, n, 1, variant, False, sch, per={"N_i": PER_N, "delta_t_i": dts})
    _has(d, [kernel])
    Uo, lamo = _oracle(m1, m2, n, PER_N, dts, variant, False, sch)
    for k in range(n):
        _check(U[k], None if lam is None else lam[k], Uo[k], None if lamo is None else lamo[k], "%s %s instance %d" % (path, name, k))


@pytest.mark.parametrize("variant", [H.DIV, H.AM_DIV], ids=["DIV", "AM_DIV"])
def test_flag_table_offset_of_the_second_sub_batch(h, variant):
    """6 instances of 256x128 cut in two halves on two streams: the second half starts at instance o = 3 and reads the flag
    table from row 3 on (div_flag + o * flag_stride).  The (N, dt) are chosen so that row k and row k + 3 differ for every k."""
    m1, m2, n = 256, 128, 6
    Ns, Ts = [6, 8, 5, 8, 5, 7], [1.0, 1.0, 0.7, 0.55, 1.0, 0.8]
    dts = [t / k for t, k in zip(Ts, Ns)]
    sch = ([0.2, 0.4, 0.6, 0.8], [0.5, 30.0, 0.2, 0.1], [0.02, 0.1, 0.02, 0.02])
    rows = [D.flags(Ns[k], dts[k], sch[0], max(Ns)) for k in range(n)]
    assert all(rows[k] != rows[k + 3] and any(f >= 0 for f in rows[k]) and any(f >= 0 for f in rows[k + 3]) for k in range(3)), rows
    with tuned(h, {"streams": 2, "team_launch": 0}):
        U, lam, d = _solve(h, m1, m2, n, 1, variant, False, sch, per={"N_i": Ns, "delta_t_i": dts})
    _has(d, ["hadi_pass_a<4,1,", "AM-P" if variant == H.AM_DIV else ",EU>", "2 sub-batches of 3 instances", "two streams"])
    Uo, lamo = _oracle(m1, m2, n, Ns, dts, variant, False, sch)
    for k in range(n):
        _check(U[k], None if lam is None else lam[k], Uo[k], None if lamo is None else lamo[k], "flag offset instance %d" % k)


# ---- the graph key: same paying steps replay, other paying steps capture --------------------------------------------------------
def test_replay_with_new_amounts():
    m1, m2, n, N = 150, 60, 2, 10
    dt = Cm.T / N
    A = D.named(N, dt, Cm.T)["canon"]
    A2 = (A[0], [25.0, 0.0, 3.0, -1.0], [0.0, 0.3, 0.05, 0.0])
    B = D.named(N, dt, Cm.T)["step1"]
    assert D.paying_steps(N, dt, A[0]) == D.paying_steps(N, dt, A2[0]) != D.paying_steps(N, dt, B[0])
    with H.HestonADI(0) as s:
        s.set_tuning("team_launch", 0)
        want = [(A, 1, 0), (A2, 0, 1), (B, 1, 0)]
        for call, (sch, captures, replays) in enumerate(want):
            g0 = Cm.graph_counts(s)
            U, _, d = _solve(s, m1, m2, n, N, H.DIV, False, sch)
            dg = Cm.graph_delta(g0, Cm.graph_counts(s))
            assert (dg["captures"], dg["replays"]) == (captures, replays), (call, dg)
            _has(d, ["hadi_pass_a<4,1,"])
            Uo, _ = _oracle(m1, m2, n, [N] * n, [dt] * n, H.DIV, False, sch)
            _check(U, None, Uo, None, "replay call %d" % (call + 1))
        # the oracle's fields of A and A' differ by far more than the bound: a replay with A's amounts would not pass
        UA, _ = _oracle(m1, m2, n, [N] * n, [dt] * n, H.DIV, False, A)
        UA2, _ = _oracle(m1, m2, n, [N] * n, [dt] * n, H.DIV, False, A2)
        assert np.abs(UA - UA2).max() > 1e-3 * np.abs(UA).max()
        Ue, _, de = _solve(s, m1, m2, n, N, H.DIV, False, ([], [], []))
        Ueu, _, deu = _solve(s, m1, m2, n, N, H.EU, False, None)
        _has(de, ["hadi_pass_a<4,1,"], ["hadi_team_kernel"])
        assert de == deu
        assert np.array_equal(Ue, Ueu)  # the dividend variant with no dividends is the plain European sweep, bit for bit
        Uo, _ = _oracle(m1, m2, n, [N] * n, [dt] * n, H.EU, False, ((), (), ()))
        _check(Ue, None, Uo, None, "replay call 4 (empty schedule)")


# ---- the American P representation around dividend steps -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["every_step", "alternate", "step1", "lastN"])
@pytest.mark.parametrize("route", ["stream1_P", "strips8"])
def test_p_representation_around_dividend_steps(h, route, name):
    """Dividend steps run on the explicit (U, lambda_bar) pair, materialised before the jump and taken back afterwards:
    `alternate` makes every other step explicit (the densest the dating rule admits -- `every_step` pays on step 1 only, see the
    module docstring), `step1` puts the jump on the step that is explicit anyway, `lastN` has the jump and its step followed by
    the final materialise.  P representation and explicit pair each against the oracle, and against each other within 2e-10
    (two fields within 1e-10 of the same third)."""
    r = ROUTES[route]
    N = r["N"]
    sch = D.named(N, Cm.T / N, Cm.T)[name]
    out = {1: _run_route(h, route, H.AM_DIV, False, name, sch, label="%s P representation %s" % (route, name)),
           0: _run_pair(h, route, name, sch)}
    scale = np.abs(out[1][0]).max()
    assert np.abs(out[1][0] - out[0][0]).max() <= 2e-10 * scale
    assert np.abs(out[1][1] - out[0][1]).max() <= 2e-8 * max(1.0, np.abs(out[1][1]).max())


def _run_pair(h, route, name, sch):
    """The route with the explicit pair in place of the P representation (describe_last_sweep() then has no AM-P)."""
    r = ROUTES[route]
    m1, m2, n, N = r["m1"], r["m2"], r["n"], r["N"]
    with tuned(h, dict(r["tune"], american_p=0)):
        U, lam, d = _solve(h, m1, m2, n, N, H.AM_DIV, False, sch)
    _has(d, [{"stream1_P": "hadi_pass_a<1,1,", "strips8": "hadi_pass_a_strip<8,AM>"}[route]], ["AM-P"])
    Uo, lamo = _oracle(m1, m2, n, [N] * n, [Cm.T / N] * n, H.AM_DIV, False, sch)
    _check(U, lam, Uo, lamo, "%s explicit pair %s" % (route, name))
    return U, lam


# ---- caller grids whose s-axis does not start at 0 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["canon", "big_cash", "negative"])
@pytest.mark.parametrize("kind", ["uniform", "geometric"])
@pytest.mark.parametrize("path,m1,m2,n,variant,put,tune,kernel", [
    ("small", 50, 25, 3, H.AM_DIV, False, {}, "hadi_small_kernel<1,"),
    ("streaming", 300, 80, 2, H.DIV, True, {"strip": 1, "team_launch": 0}, "hadi_pass_a_strip<8,EU>"),
    ("team", 300, 80, 2, H.DIV, False, {"team_launch": 1}, "hadi_team_kernel<8>")], ids=["small", "streaming", "team"])
def test_caller_grids_that_do_not_start_at_zero(h, path, m1, m2, n, variant, put, tune, kernel, kind, name):
    """s-axis on [10, 400], uniform and geometric: ex-dividend spots with 0 < new_s < s_0 find node 0 as the first node above
    them and take its value (canon, big_cash); `negative` lifts the top nodes above s_max into the same branch."""
    N = 10
    dt = Cm.T / N
    sch = D.named(N, dt, Cm.T)[name]
    for paid, counts in _require(name, N, dt, sch, m1, m2, n, put, kind):
        tot = D.total(counts)
        assert (tot.fallback - tot.below_s0 >= 1) if name == "negative" else (tot.below_s0 >= 1), (name, counts)
    with tuned(h, tune):
        U, lam, d = _solve(h, m1, m2, n, N, variant, put, sch, kind=kind)
    _has(d, [kernel])
    Uo, lamo = _oracle(m1, m2, n, [N] * n, [dt] * n, variant, put, sch, kind=kind)
    _check(U, lam, Uo, lamo, "%s %s grid %s" % (path, kind, name))


# ---- Greeks: theta reads the state that the last jump and step left behind -------------------------------------------------------
@pytest.mark.parametrize("name", ["big_cash", "step1"])
@pytest.mark.parametrize("m1,m2,tune,kernel", [(50, 25, {}, "hadi_small_kernel<1,8,EU>"), (300, 80, {"strip": 1, "team_launch": 0}, "hadi_pass_a_strip<8,EU>")],
                         ids=["50x25", "300x80"])
def test_greeks_with_schedules(h, m1, m2, tune, kernel, name):
    n, N = 2, 10
    dt = Cm.T / N
    sch = D.named(N, dt, Cm.T)[name]
    _require(name, N, dt, sch, m1, m2, n)
    strikes, grids, U0 = _inputs(m1, m2, n)
    V0 = Cm.v0_for(m2)
    with tuned(h, tune):
        greeks, lad = h.compute_greeks(m1, m2, N, dt, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U0.copy(),
                                       Cm.S_0, V0, variant=H.DIV, dividends=H.Dividends(*sch), ladder=True)
        _has(h.describe_last_sweep(), [kernel])
    for k in range(n):
        g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
        p = O.make_params(m1, m2, N, dt, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.DIV, sch)
        b, U, _ = G.boundary_vector(p, *g, U0[k])
        j0, i0 = G.find_node(g[1], V0), G.find_node(g[0], Cm.S_0)
        assert i0 >= 0 and j0 >= 0
        ref = G.ladder(p, *g, U, None, j0, b)
        bound = G.propagated_bound(p, g[0], g[1], j0, np.abs(U).max())
        r, where = G.worst_ratio(lad[k], ref, bound)
        print("greeks %dx%d %s instance %d: worst |diff| / bound %.3e at node %d column %s" % (m1, m2, name, k, r, where[0], G.NAMES[where[1]]))
        assert r <= 1.0, (k, where, lad[k][where], ref[where], bound[where])
        assert np.array_equal(greeks[k], lad[k, i0])


# ---- seeded random campaign ------------------------------------------------------------------------------------------------------
CAMPAIGN_ROUTES = [r for r in ROUTES if r != "seq_passes"]


@pytest.mark.parametrize("seed", range(40))
def test_random_schedules_on_rotating_paths(h, seed):
    rng = random.Random(9100 + seed)
    route = rng.choice(CAMPAIGN_ROUTES)
    r = ROUTES[route]
    american = rng.random() < 0.5 and r["kernel"][True] is not None
    put = rng.random() < 0.5
    N = rng.randint(3, 20 if r["m1"] <= 150 else 10)
    sch = D.random_schedule(rng, N, Cm.T / N)
    while not D.paying_steps(N, Cm.T / N, sch[0]):  # (a schedule that pays nothing would make the case the plain sweep)
        sch = D.random_schedule(rng, N, Cm.T / N)
    assert D.paying_steps(N, Cm.T / N, sch[0]), (seed, sch)
    label = "seed %d: %s %s %s N = %d, pays %r" % (seed, route, "AM_DIV" if american else "DIV", "put" if put else "call", N,
                                                   D.paying_steps(N, Cm.T / N, sch[0]))
    _run_route(h, route, H.AM_DIV if american else H.DIV, put, None, sch, N=N, label=label)
