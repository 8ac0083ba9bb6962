"""CPU-only: every kernel family of the wave emulator at the rate regimes R0 .. R7 and the model regimes M0 .. M8 of
tests/regimes.py.  The rest of the emulator suite runs r_d = 0.025 and a narrow model box; here r_d is 0, negative and large,
q = r_d - r_f is 0 (the strips must be refused), tiny (the strips' A0 weights divided by theta dt q are ~1e14) and of either
sign, rho is 0 (A0 empty) and +-1, the variance is nearly deterministic, without mean reversion and convection-dominated.  A
rate regime is one call on the canonical model; the model regimes travel per instance, three to a batch, rotated by the class
index so that neighbours never share a model.  Bounds: test_emu_kernel_logic._run (1e-11 max|U_ref|, lambda_bar 1e-9), 1e-10
for the resident sweep and the small scheme kernel as in their own files.  The power-of-two spot scaling is held bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import regimes as R
import scheme_ref as S
import test_emu_small_sch as ES
from test_emu_kernel_logic import _P, _plan, emu  # noqa: F401  (emu: the module's fixture)
from test_emu_resident import emu as emu_resident  # noqa: F401
from test_emu_small_sch import emu as emu_small_sch  # noqa: F401

EMU_AMP = 3
TOL = 1e-11

#          id                   tuning                           m1   m2  N   variant   tw keywords                  plan (B, G, strips, pairs)
CLASSES = [("ring_one_node",     {},                              40,  12, 3,  O.EU,     8, {},                       (1, 1, False, False)),
           ("ring_two_nodes",    {},                              100, 20, 2,  O.AM,     8, {},                       (2, 1, False, False)),
           ("ring_eight_nodes",  {},                              300, 12, 2,  O.EU,     8, {},                       (8, 1, False, False)),
           ("ring_put",          {},                              40,  12, 3,  O.EU,     8, dict(put=True),           (1, 1, False, False)),
           ("strips",            {"strip": 1},                    300, 40, 2,  O.EU,     1, {},                       (8, 1, True, False)),
           ("strips_forced_am",  {"strip": 1},                    280, 40, 2,  O.AM,     1, {},                       (8, 1, True, False)),
           ("strips_put_am",     {"strip": 1},                    300, 40, 2,  O.AM,     1, dict(put=True),           (8, 1, True, False)),
           ("pairs",             {"strip": 1, "pair_strips": 1},  256, 54, 2,  O.EU,     1, {},                       (4, 1, True, True)),
           ("paired_strips",     {"strip": 1},                    600, 26, 2,  O.EU,     1, {},                       (8, 2, True, False)),
           ("two_wave_ring",     {},                              600, 12, 2,  O.EU,     8, {},                       (8, 2, False, False)),
           ("american_p_strips", {"strip": 1},                    300, 70, 2,  O.AM,     1, dict(scheme=EMU_AMP),     (8, 1, True, False)),
           ("dividends_strips",  {"strip": 1},                    200, 60, 10, O.AM_DIV, 1, {},                       (4, 1, True, False)),
           ("small_block",       {},                              50,  25, 6,  O.AM_DIV, 8, dict(small=1),            None),
           ("small_block_put",   {},                              40,  12, 4,  O.EU,     8, dict(small=1, put=True),  None),
           ("small_seq",         {},                              50,  25, 3,  O.EU,     8, dict(small=3),            None),
           ("small_seq2",        {},                              50,  25, 3,  O.EU,     8, dict(small=5),            None),
           ("small_seq2_div_put", {},                             40,  12, 12, O.DIV,    8, dict(small=5, put=True),  None),
           ("team",              {},                              300, 40, 2,  O.EU,     8, dict(small=4),            None),
           ("team_put",          {},                              300, 40, 2,  O.EU,     8, dict(small=4, put=True),  None),
           ("team_div",          {},                              200, 40, 6,  O.DIV,    8, dict(small=4),            None)]
# (The three team rows are solved at 6 of the 8 rate regimes: at R0 and R7, q = 0, the library keeps the team kernel off and
# emu_solve refuses the call as hadi_api.hip does -- those six cases assert the refusal, rc == 3, and compute nothing.  The
# model batches are rotated by c = class index, not by a rate-regime index: the rate cases run on M0 throughout.)
INDEX = {c[0]: k for k, c in enumerate(CLASSES)}
REGIME_RUNS = [r[0] for r in R.RATES] + ["M%d-M%d" % (a, a + 2) for a in (0, 3, 6)]


def _inputs(m1, m2, n, put):
    strikes = Cm.well_conditioned_strikes(m1, n)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    if put:
        U0 = Cm.put_payoff(vs, strikes, m2)
    return strikes, vs, vv, ds, dv, U0


def _setup(run, cls_index):
    """(r_d, r_f, models of the batch): a rate regime on two instances of M0, or three model regimes rotated by the class."""
    if run in R.RATE:
        return R.RATE[run] + ([R.CANONICAL_MODEL] * 2,)
    first = int(run[1])
    return R.MODEL_RATES + ([R.MODELS[(first + k + cls_index) % 9][1:] for k in range(3)],)


def _emu(emu, m1, m2, N, variant, tw, r_d, r_f, models, grids, small=0, scheme=0, put=False, divs=Cm.DIVS):
    strikes, vs, vv, ds, dv, U0 = grids
    n = len(strikes)
    ks = np.array(strikes, dtype=np.float64)
    U, lam = U0.copy(), np.zeros_like(U0)
    par = np.ascontiguousarray(np.array(models, dtype=np.float64).reshape(n, 4))
    dd = [np.array(x, dtype=np.float64) for x in divs]
    rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(r_d), C.c_double(r_f), _P(par),
                       variant, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), _P(U0), _P(lam), tw, len(dd[0]), _P(dd[0]), _P(dd[1]),
                       _P(dd[2]), 64, small, scheme, _P(ks) if put else None, None, None)
    if small == 4 and r_d == r_f:
        assert rc == 3, rc  # the library keeps the team kernel off without r_d - r_f, as it does the strips (hadi_api.hip, team_shape)
        return None, None
    assert rc == 0, rc
    return U, lam


def _oracle(m1, m2, N, variant, r_d, r_f, model, grids, k, put, divs=Cm.DIVS):
    strikes, vs, vv, ds, dv, U0 = grids
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, r_d, r_f, *model, variant, divs if variant in (O.DIV, O.AM_DIV) else None,
                      option_type=O.PUT if put else O.CALL, strikes=np.array(strikes[k:k + 1]) if put else None)
    Uo, lo, _ = O.solve(p, vs[k], vv[k], ds[k], dv[k], U0[k], U0[k])
    assert np.isfinite(Uo).all()
    return Uo, lo


class _tuning:
    def __init__(self, emu, tuning):
        self.emu, self.tuning = emu, tuning

    def __enter__(self):
        for k, v in self.tuning.items():
            assert self.emu.emu_set_tuning(k.encode(), v) == 0

    def __exit__(self, *exc):
        self.emu.emu_set_tuning(b"reset", 0)


@pytest.mark.parametrize("run", REGIME_RUNS)
@pytest.mark.parametrize("name,tuning,m1,m2,N,variant,tw,kw,plan", CLASSES, ids=[c[0] for c in CLASSES])
def test_family_at_regime(emu, name, tuning, m1, m2, N, variant, tw, kw, plan, run):
    r_d, r_f, models = _setup(run, INDEX[name])
    n, put = len(models), kw.get("put", False)
    grids = _inputs(m1, m2, n, put)
    with _tuning(emu, tuning):
        assert plan is None or _plan(emu, m1, m2, n, tw) == plan, (_plan(emu, m1, m2, n, tw), plan)
        U, lam = _emu(emu, m1, m2, N, variant, tw, r_d, r_f, models, grids, **kw)
    if U is None:
        assert run in R.Q_ZERO and kw.get("small") == 4
        return
    worst = wl = 0.0
    for k in range(n):
        Uo, lo = _oracle(m1, m2, N, variant, r_d, r_f, models[k], grids, k, put)
        worst = max(worst, np.abs(U[k] - Uo).max() / np.abs(Uo).max())
        if lo is not None:
            wl = max(wl, np.abs(lam[k] - lo).max() / max(1.0, np.abs(lo).max()))
    print("%s %s: field %.2e, lambda_bar %.2e" % (name, run, worst, wl))
    assert worst < TOL and wl < 1e-9, (worst, wl)


def test_every_rate_and_model_regime_is_in_the_runs():
    """The run list really reaches all 17 regimes on every class, whatever the class index."""
    for c in range(len(CLASSES)):
        seen = {m for run in REGIME_RUNS if run not in R.RATE for m in _setup(run, c)[2]}
        assert seen == {m[1:] for m in R.MODELS}
    assert {r for r in REGIME_RUNS if r in R.RATE} == set(R.RATE)
    want = {"ring_one_node", "ring_two_nodes", "ring_eight_nodes", "strips", "strips_forced_am", "pairs", "paired_strips",
            "two_wave_ring", "american_p_strips", "dividends_strips", "small_block", "small_seq", "small_seq2", "team"}
    assert want <= set(INDEX)


# ---- the resident sweep -------------------------------------------------------------------------------------------------
def _resident(emu_resident, m1, m2, N, r_d, r_f, models, grids, put=False):
    strikes, vs, vv, ds, dv, U0 = grids
    n = len(strikes)
    par = np.ascontiguousarray(np.array(models, dtype=np.float64).reshape(n, 4))
    ks = np.ascontiguousarray(strikes, dtype=np.float64)
    U, P = U0.copy(), C.c_int(0)
    rc = emu_resident.emu_solve_resident(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(Cm.THETA), C.c_double(r_d), C.c_double(r_f),
                                         _P(par), _P(vs), _P(vv), _P(ds), _P(dv), _P(U), 64, None, None, C.byref(P), _P(ks),
                                         1 if put else 0)
    return rc, U


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
@pytest.mark.parametrize("run", REGIME_RUNS)
def test_resident_sweep_at_regime(emu_resident, run, put):
    m1, m2, N = 300, 40, 2
    r_d, r_f, models = _setup(run, len(CLASSES) + put)
    grids = _inputs(m1, m2, len(models), put)
    rc, U = _resident(emu_resident, m1, m2, N, r_d, r_f, models, grids, put)
    if run in R.Q_ZERO:
        assert rc == 3  # no strips without r_d - r_f, and no resident sweep without strips
        return
    assert rc == 0, rc
    worst = max(np.abs(U[k] - Uo).max() / np.abs(Uo).max()
                for k in range(len(models)) for Uo in [_oracle(m1, m2, N, O.EU, r_d, r_f, models[k], grids, k, put)[0]])
    print("resident %s %s: field %.2e" % (run, "put" if put else "call", worst))
    assert worst <= 1e-10  # (the bound of test_emu_resident._check)


# ---- hadi_small_sch_kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", REGIME_RUNS)
@pytest.mark.parametrize("scheme,theta,name", ES.SCHEMES, ids=[s[2] for s in ES.SCHEMES])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 20)], ids=["50x25", "100x20"])
def test_small_scheme_kernel_at_regime(emu_small_sch, m1, m2, scheme, theta, name, run):
    N = 2
    r_d, r_f, models = _setup(run, scheme + (m1 > 64))
    n = len(models)
    strikes, vs, vv, ds, dv, U0 = _inputs(m1, m2, n, False)
    par8 = np.array([list(models[k]) + [Cm.T / N, N, 0.0, 0.0] for k in range(n)])
    U = np.ascontiguousarray(U0.copy())
    rc = emu_small_sch.emu_small_sch(n, m1, m2, C.c_double(theta), C.c_double(r_d), C.c_double(r_f), _P(par8), _P(vs), _P(vv),
                                     _P(ds), _P(dv), _P(U), scheme, 64, None)
    assert rc == 0, rc
    worst = 0.0
    for k in range(n):
        p = O.make_params(m1, m2, N, Cm.T / N, theta, r_d, r_f, *models[k], O.EU)
        Uo = S.solve_one(p, vs[k], vv[k], ds[k], dv[k], U0[k], scheme)
        assert np.isfinite(Uo).all()
        worst = max(worst, np.abs(U[k] - Uo).max() / np.abs(Uo).max())
    print("small_sch %s %dx%d %s: field %.2e" % (name, m1, m2, run, worst))
    assert worst <= 1e-10  # (the bound of test_emu_small_sch._check)


# ---- power-of-two spot scaling, bit for bit -----------------------------------------------------------------------------
SCALING = [("ring_one_node", O.AM_DIV, False, 10), ("small_block", O.DIV, True, 12), ("strips", O.AM, True, 2), ("strips", O.EU, False, 2),
           ("two_wave_ring", O.EU, False, 2), ("team", O.EU, True, 2)]


@pytest.mark.parametrize("name,variant,put,N", SCALING, ids=["%s_v%d_%s" % (s[0], s[1], "put" if s[2] else "call") for s in SCALING])
def test_spot_scaling_is_exact(emu, name, variant, put, N):
    """vec_s, delta_s, strikes, payoff and dividend amounts times 2^k give exactly 2^k times the field and lambda_bar."""
    _, tuning, m1, m2, _, _, tw, kw, _ = CLASSES[INDEX[name]]
    kw = {**kw, "put": put}
    r_d, r_f = R.MODEL_RATES
    models = [R.MODEL["M0"], R.MODEL["M8"]]
    grids = _inputs(m1, m2, 2, put)
    strikes, vs, vv, ds, dv, U0 = grids
    american = variant in (O.AM, O.AM_DIV)
    with _tuning(emu, tuning):
        U, lam = _emu(emu, m1, m2, N, variant, tw, r_d, r_f, models, grids, **kw)
        assert not american or np.abs(lam).max() > 0
        for k in R.SCALE_POWERS:
            vs2, ds2, U02, ks2, divs2 = R.scaled(k, vs, ds, U0, strikes, Cm.DIVS)
            Us, ls = _emu(emu, m1, m2, N, variant, tw, r_d, r_f, models, (ks2, vs2, vv, ds2, dv, U02), divs=divs2, **kw)
            assert np.array_equal(Us, U * 2.0 ** k), (name, k)
            assert not american or np.array_equal(ls, lam * 2.0 ** k), (name, k)
