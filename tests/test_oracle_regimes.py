"""CPU-only: the footing of the regime tests (tests/regimes.py).  At every rate regime R0 .. R7 and model regime M0 .. M8 the
fp64 oracle sits on its binary128 twin to round-off -- so the project's bounds (field 1e-10 max|U_ref|, lambda_bar 1e-8) keep
their margin over the reference's own error there -- every regime moves the field by far more than any bound (a kernel that
read the wrong rate or model cannot pass), and the oracle is exactly homogeneous in the spot scale for powers of two."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import regimes as R

SHAPES = [(50, 25, 20), (300, 40, 4), (600, 30, 3)]
#            id          variant   put
VARIANTS = [("eu_call",   O.EU,     False), ("am_put", O.AM, True), ("amdiv_call", O.AM_DIV, False)]
REGIMES = [(r[0], (r[1], r[2]), R.CANONICAL_MODEL) for r in R.RATES] + [(m[0], R.MODEL_RATES, m[1:]) for m in R.MODELS]
FIELD_XP, LAMBDA_XP = 5e-12, 1e-9  # (lambda_bar: the bound of test_oracle_xp.py)
SENSITIVITY = 1e-6


@functools.lru_cache(maxsize=None)
def _inputs(m1, m2, put):
    K = Cm.well_conditioned_strikes(m1, 1)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, K, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    if put:
        U0 = Cm.put_payoff(vs, K, m2)
    return K, vs[0], vv[0], ds[0], dv[0], U0[0]


def _params(m1, m2, N, variant, put, rates, model, K, divs=Cm.DIVS):
    return O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, *rates, *model, variant, divs if variant in (O.DIV, O.AM_DIV) else None,
                         option_type=O.PUT if put else O.CALL, strikes=np.array(K) if put else None)


@functools.lru_cache(maxsize=None)
def _field(m1, m2, N, variant, put, rates, model):
    K, *g = _inputs(m1, m2, put)
    U, lam, _ = O.solve(_params(m1, m2, N, variant, put, rates, model, K), *g, g[-1])
    assert np.isfinite(U).all()
    return U, lam


@pytest.mark.parametrize("rid,rates,model", REGIMES, ids=[r[0] for r in REGIMES])
@pytest.mark.parametrize("vid,variant,put", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_oracle_sits_on_its_binary128_twin(m1, m2, N, vid, variant, put, rid, rates, model):
    K, *g = _inputs(m1, m2, put)
    U, lam = _field(m1, m2, N, variant, put, rates, model)
    Ux, lx = O.solve_xp(_params(m1, m2, N, variant, put, rates, model, K), *g, g[-1])
    assert np.isfinite(Ux).all()
    e = np.abs(U - Ux).max() / np.abs(Ux).max()
    el = 0.0 if lam is None else np.abs(lam - lx).max() / max(1.0, np.abs(lx).max())
    print("%s %s %dx%dx%d: field %.2e, lambda_bar %.2e" % (rid, vid, m1, m2, N, e, el))
    assert e <= FIELD_XP and el <= LAMBDA_XP, (e, el)


MOVING = [r for r in REGIMES if r[0] != "M0"]  # (M0 is the field the model regimes are compared with)


@pytest.mark.parametrize("rid,rates,model", MOVING, ids=[r[0] for r in MOVING])
@pytest.mark.parametrize("vid,variant,put", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("m1,m2,N", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_every_regime_moves_the_field(m1, m2, N, vid, variant, put, rid, rates, model):
    """Against the canonical rates (rate regimes) or M0 at the model regimes' rates (model regimes): >= 1e-6 of max|U|.  R6 is
    q ~ -2.5e-14 beside r_f = r_d: it is there for the strips' scaling, so it is held against the canonical field like the
    others, NOT against the field of r_f = r_d, which it equals to round-off."""
    base = R.CANONICAL_RATES if rid.startswith("R") else R.MODEL_RATES
    U, _ = _field(m1, m2, N, variant, put, rates, model)
    Uc, _ = _field(m1, m2, N, variant, put, base, R.CANONICAL_MODEL)
    d = np.abs(U - Uc).max() / np.abs(Uc).max()
    print("%s %s %dx%dx%d: %.2e of max|U| from the canonical field" % (rid, vid, m1, m2, N, d))
    assert d >= SENSITIVITY, d


def test_r6_equals_equal_rates_to_round_off_but_not_bit_for_bit_in_q():
    """What R6 is: r_d - r_f is a non-zero fp64 number (the host keeps the strips), the field is the one of r_f = r_d."""
    r_d, r_f = R.RATE["R6"]
    assert r_d - r_f != 0.0 and abs(r_d - r_f) < 1e-13
    U, _ = _field(300, 40, 4, O.EU, False, (r_d, r_f), R.CANONICAL_MODEL)
    Ue, _ = _field(300, 40, 4, O.EU, False, (r_d, r_d), R.CANONICAL_MODEL)
    assert np.abs(U - Ue).max() <= 1e-11 * np.abs(Ue).max()


SCALING = [("eu_call", O.EU, False), ("div_put", O.DIV, True), ("am_put", O.AM, True), ("amdiv_call", O.AM_DIV, False)]


@pytest.mark.parametrize("k", R.SCALE_POWERS)
@pytest.mark.parametrize("vid,variant,put", SCALING, ids=[v[0] for v in SCALING])
def test_power_of_two_spot_scaling_is_exact(vid, variant, put, k):
    """vec_s, delta_s, strike, payoff and dividend amounts times 2^k: the field and lambda_bar are 2^k times the unscaled ones,
    bit for bit (every product with the spot axis is a power-of-two rescaling; the operators are homogeneous of degree 0)."""
    m1, m2, N = 50, 25, 20
    K, vs, vv, ds, dv, U0 = _inputs(m1, m2, put)
    U, lam = _field(m1, m2, N, variant, put, R.MODEL_RATES, R.CANONICAL_MODEL)
    vs2, ds2, U02, K2, divs2 = R.scaled(k, vs, ds, U0, K, Cm.DIVS)
    Us, ls, _ = O.solve(_params(m1, m2, N, variant, put, R.MODEL_RATES, R.CANONICAL_MODEL, K2, divs2), vs2, vv, ds2, dv, U02, U02)
    assert np.array_equal(Us, U * 2.0 ** k)
    assert lam is None or (np.array_equal(ls, lam * 2.0 ** k) and np.abs(lam).max() > 0)
