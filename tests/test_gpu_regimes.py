"""Every kernel family, variant, scheme and launcher at the rate regimes R0 .. R7 and the model regimes M0 .. M8 of
tests/regimes.py, and under power-of-two spot scaling.

The rest of the GPU suite runs r_d = 0.025 throughout, r_f from a handful of values and (rho, sigma, kappa, eta) from a narrow
box, strikes 80 .. 120.  These inputs select code paths: q = r_d - r_f, half_rd, bc_rate = put ? -r_d : r_f and hr0 per
instance (hadi_core.h), the strips' A0 weights divided by -theta dt q (~1e14 at R6; at q = 0 the host must keep the strips, the
team kernel and the resident sweep off), the team kernel's unit_e branch at bc_rate == 0 (with put data: r_d = 0, R1), rho = 0
(A0 empty), a convection-dominated v-direction for the un-pivoted pentadiagonal LU (M7).  What the emulator cannot show is the
gfx950 build: the reciprocal with its Newton step, device exp, contraction.

No new launch configuration: rows, tuning keys and kernel names are those of test_gpu_mixed_vgrids.py (FAMILIES, VARIANTS,
SCHEMES, the team and resident cases).  A rate regime is one call on the canonical model through the scalars; the model regimes
travel per instance (rho_i .. eta_i), instance k of a batch on model (k + c) % 9 for c = 0, n, 2n, .. so that every model meets
every row and neighbours never share one; one more call per row passes a single non-canonical model through the scalars.
Bounds are the project's: field 1e-10 max|U_ref| per instance on well-conditioned grids (asserted), fp32 state 2e-7 N,
lambda_bar 1e-8 max(1, max|lambda|), prices 1e-9, J 2e-4, Greeks at the propagated bound of tests/greeks_ref.py.  Every case
asserts from describe_last_sweep() which kernel ran, that its reference is finite and that the regime moved the reference by
>= 1e-6 of max|U| from the canonical one, and prints its observed maximum."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm
import greeks_ref as G
import regimes as R
import scheme_ref as S
from test_gpu_mixed_vgrids import FAMILIES, OV, RESIDENT, SCHEMES, SMALL_SCH, VARIANTS, _check, _has, _st, _tuned

pytestmark = pytest.mark.gpu

M0 = R.CANONICAL_MODEL
RATE_IDS = [r[0] for r in R.RATES]
TEAM = [("team_300x140", 300, 140, 3, 3, H.EU, "hadi_team_kernel<8>"), ("team_256x128_div", 256, 128, 10, 8, H.DIV, "hadi_team_kernel<4>")]
RES = (300, 80, 256)
SUBSET = (0, 1, 7, 8, 254, 255)


def _v0(m2):
    """V_0 of the shared v-grid: the canonical 0.04 unless its grid breaks the 30x rule at this m2 (every batch asserts it)."""
    return next(v for v in (Cm.V_0, Cm.V_0_ALT) if Cm.interval_ratios(O.rebuild_variance(m2, v)[1])[0] <= Cm.COND_MAX)


@functools.lru_cache(maxsize=None)
def _inputs(m1, m2, n, put=False):
    """(strikes, grids, U0, V_0): n well-conditioned strikes on one well-conditioned v-grid; built once, left unchanged."""
    strikes = tuple(Cm.well_conditioned_strikes(m1, n))
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, _v0(m2), strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    U0.setflags(write=False)
    return strikes, grids, U0, _v0(m2)


def _scaled_inputs(m1, m2, n, put, k):
    """The batch with the spot axis, the payoff, the strikes and the dividend amounts times 2^k (k = 0: as it is)."""
    strikes, grids, U0, v0 = _inputs(m1, m2, n, put)
    if k == 0:
        return strikes, grids, U0, Cm.DIVS
    _, _, U0s, ks, divs = R.scaled(k, grids.Vec_s, grids.Delta_s, U0, strikes, Cm.DIVS)
    return tuple(ks), Cm.spot_scaled_grids(grids, k), U0s, divs


def _models(n, c):
    return tuple(R.rotating_models(n, c))


def _rotations(n):
    """The c of the model batches of an n-instance row: instance k on model (k + c) % 9, every model on some instance."""
    cs = list(range(0, len(R.MODELS), n))
    assert {m for c in cs for m in _models(n, c)} == {m[1:] for m in R.MODELS}
    return cs


def _sweep(sv, tuning, m1, m2, N, n, r_d, r_f, models, variant=H.EU, put=False, scheme=0, theta=Cm.THETA, fp32=False, k=0):
    """One DO_timestepping under `tuning` -> (U_T, lambda_bar_T or None, description).  A batch of ONE model goes through the
    scalars (rho_i .. eta_i = NULL), a batch of several through the per-instance arrays (the scalars then hold instance 0's)."""
    strikes, grids, U0, divs = _scaled_inputs(m1, m2, n, put, k)
    american = variant in (H.AM, H.AM_DIV)
    U, lam = U0.copy(), (np.zeros_like(U0) if american else None)
    per = None if len(set(models)) == 1 else R.per_instance(models)
    with _tuned(sv, tuning):
        sv.DO_timestepping(m1, m2, N, Cm.T / N, theta, r_d, r_f, *models[0], grids, U, variant=variant,
                           U_0=U0.copy() if american else None, lambda_bar=lam,
                           dividends=H.Dividends(*divs) if variant in (H.DIV, H.AM_DIV) else None, per_instance=per, scheme=scheme,
                           state_precision=H.STATE_FP32 if fp32 else H.STATE_FP64, option_type=H.PUT if put else H.CALL,
                           strikes=list(strikes) if put else None)
        d = sv.describe_last_sweep()
        state = sv.get_tuning("team_launch")
    assert tuning.get("team_launch") != 1 or state == 1, (d, state)  # (the team protocol did not fail)
    return U, lam, d


@functools.lru_cache(maxsize=12)
def _reference(m1, m2, N, n, r_d, r_f, models, variant=H.EU, put=False, scheme=0, theta=Cm.THETA, fp32=False, k=0, rows=None):
    """Every instance (or `rows`) with ITS model: the oracle on 16 threads (Douglas, Craig-Sneyd), tests/scheme_ref.py (MCS, HV).
    Finite, asserted.  Computed once per case and left unchanged."""
    strikes, g, U0, divs = _scaled_inputs(m1, m2, n, put, k)
    r = list(range(n)) if rows is None else list(rows)
    ov = OV[variant]

    def params(i):
        return O.make_params(m1, m2, N, Cm.T / N, theta, r_d, r_f, *models[i], ov, divs if ov in (O.DIV, O.AM_DIV) else None,
                             scheme=1 if scheme == H.SCHEME_CRAIG_SNEYD else 0, state_fp32=1 if fp32 else 0,
                             option_type=O.PUT if put else O.CALL, strikes=np.asarray(strikes, dtype=np.float64)[[i]] if put else None)

    O.lib()
    if len(set(models)) == 1 and scheme not in (H.SCHEME_MCS, H.SCHEME_HV):
        p = params(0)
        if put:
            p = O.make_params(m1, m2, N, Cm.T / N, theta, r_d, r_f, *models[0], ov, divs if ov in (O.DIV, O.AM_DIV) else None,
                              scheme=p.scheme, state_fp32=p.state_fp32, option_type=O.PUT, strikes=np.asarray(strikes, dtype=np.float64)[r])
        Uo, lo, _ = O.solve_batch(p, g.Vec_s[r], g.Vec_v[r], g.Delta_s[r], g.Delta_v[r], U0[r], U0[r], threads=16, want_lambda=True)
    else:
        def one(i):
            a = (g.Vec_s[i], g.Vec_v[i], g.Delta_s[i], g.Delta_v[i], U0[i])
            if scheme in (H.SCHEME_MCS, H.SCHEME_HV):
                return S.solve_one(params(i), *a, S.MCS if scheme == H.SCHEME_MCS else S.HV), None
            return O.solve(params(i), *a, U0[i])[:2]
        with ThreadPoolExecutor(16) as ex:
            out = list(ex.map(one, r))
        Uo = np.stack([o[0] for o in out])
        lo = None if out[0][1] is None else np.stack([o[1] for o in out])
    assert np.isfinite(Uo).all() and (lo is None or np.isfinite(lo).all())
    Uo.setflags(write=False)
    return Uo, lo


def _assert_moved(Uo, m1, m2, N, n, r_d, r_f, models, rows=None, **kw):
    """The condition under the whole file: every instance's reference differs from the canonical-parameter one by >= 1e-6 of
    max|U| (rate regimes: canonical rates; model regimes: M0 at the same rates, instances ON M0 exempt) -- a kernel that read the
    wrong rate or model cannot pass."""
    base = R.CANONICAL_RATES if set(models) == {M0} else (r_d, r_f)
    Uc, _ = _reference(m1, m2, N, n, *base, (M0,) * n, rows=rows, **kw)
    moved = np.abs(Uo - Uc).max(axis=1) / np.abs(Uc).max(axis=1)
    idx = range(n) if rows is None else rows
    need = [j for j, i in enumerate(idx) if models[i] != M0 or base != (r_d, r_f)]
    assert need and moved[need].min() >= 1e-6, moved


def _run(sv, name, tuning, want, absent, m1, m2, N, n, r_d, r_f, models, rows=None, **kw):
    U, lam, d = _sweep(sv, tuning, m1, m2, N, n, r_d, r_f, models, **kw)
    _has(d, want, absent)
    Uo, lo = _reference(m1, m2, N, n, r_d, r_f, models, rows=rows, **kw)
    _assert_moved(Uo, m1, m2, N, n, r_d, r_f, models, rows=rows, **kw)
    sel = slice(None) if rows is None else list(rows)
    _check(name, U[sel], None if lam is None else lam[sel], Uo, lo, bound=2e-7 * N if kw.get("fp32") else 1e-10)
    return U, Uo


def _off_strips(want, absent):
    """What a strip, pairs or paired-strip row must describe at q = 0: the shared-ring kernel of its nodes-per-lane class and
    no "strip" (the assertion of test_gpu_schemes.py::test_theta_and_rates).  Other rows: unchanged."""
    s = next((w for w in want if "hadi_pass_a_strip" in w or "hadi_pass_a_pairs" in w), None)
    if s is None:
        return want, absent
    if "pairs" in s:
        B, Gw = 4, 1
    else:
        B, Gw = int(s.split("<")[1].split(",")[0]), 2 if s.rstrip(">").endswith(",2") else 1
    ring = ["hadi_pass_a<%d,%d," % (B, Gw)] + [t for t in ("AM-P", "float") if t in s]
    return ring, sorted(set(absent) | {"strip", "pairs"})


def _named(want, absent, rid):
    return _off_strips(want, absent) if rid in R.Q_ZERO else (want, absent)


def _need_256(sv):
    if sv.device_info()["compute_units"] != 256:
        pytest.skip("needs the 256-CU device")


# ---- a. Douglas families x rates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RATE_IDS)
@pytest.mark.parametrize("name,m1,m2,n,tuning,want,absent,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_family_at_rate(solver, name, m1, m2, n, tuning, want, absent, kw, rid):
    w, a = _named(want, absent, rid)
    _run(solver, "%s %s" % (name, rid), tuning, w, a, m1, m2, 3, n, *R.RATE[rid], (M0,) * n, **kw)


# ---- b. Douglas families, team kernel and resident sweep x models ---------------------------------------------------------
FAMILY_MODELS = [(f, c) for f in FAMILIES for c in _rotations(f[3])]


@pytest.mark.parametrize("fam,c", FAMILY_MODELS, ids=["%s-c%d" % (f[0], c) for f, c in FAMILY_MODELS])
def test_family_with_rotating_models(solver, fam, c):
    name, m1, m2, n, tuning, want, absent, kw = fam
    _run(solver, "%s models c=%d" % (name, c), tuning, want, absent, m1, m2, 3, n, *R.MODEL_RATES, _models(n, c), **kw)


@pytest.mark.parametrize("k", range(len(FAMILIES)), ids=[f[0] for f in FAMILIES])
def test_family_with_one_model_through_the_scalars(solver, k):
    """*_i = NULL: the scalar staging path, on a non-canonical model (M1 .. M8 in turn by family index)."""
    name, m1, m2, n, tuning, want, absent, kw = FAMILIES[k]
    mid, *model = R.MODELS[1 + k % 8]
    _run(solver, "%s scalar %s" % (name, mid), tuning, want, absent, m1, m2, 3, n, *R.MODEL_RATES, (tuple(model),) * n, **kw)


TEAM_MODELS = [(t, c) for t in TEAM for c in _rotations(t[4])]


@pytest.mark.parametrize("team,c", TEAM_MODELS, ids=["%s-c%d" % (t[0], c) for t, c in TEAM_MODELS])
def test_team_kernel_with_rotating_models(solver, team, c):
    _need_256(solver)
    name, m1, m2, N, n, variant, kernel = team
    _run(solver, "%s models c=%d" % (name, c), {"team_launch": 1}, [kernel], [], m1, m2, N, n, *R.MODEL_RATES, _models(n, c), variant=variant)


def _resident_pair(sv, name, N, r_d, r_f, models, stays=True, **kw):
    """"resident_sweep" = 1 and again 0, as test_gpu_resident.py::test_inputs: the two fields to 1e-13, the resident one against
    the oracle (every instance) at 1e-10."""
    m1, m2, n = RES
    U, Uo = _run(sv, name, {"resident_sweep": 1}, [RESIDENT, "hadi_pass_a_strip<8,EU> (strips of 11 rows)"] if stays else [], [] if stays else [RESIDENT],
                 m1, m2, N, n, r_d, r_f, models, **kw)
    Us, _, ds = _sweep(sv, {"resident_sweep": 0}, m1, m2, N, n, r_d, r_f, models, **kw)
    _has(ds, [], [RESIDENT])
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("  resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13 and np.isfinite(U).all()
    return U


@pytest.mark.parametrize("c", [0, 5])
def test_resident_sweep_with_rotating_models(solver, c):
    _need_256(solver)
    _resident_pair(solver, "resident models c=%d" % c, 4, *R.MODEL_RATES, _models(RES[2], c))


# ---- c. variants x rates and models ---------------------------------------------------------------------------------------
VARIANT_RUNS = [(v, rid) for v in VARIANTS for rid in RATE_IDS + ["c%d" % c for c in _rotations(4)]]


@pytest.mark.parametrize("var,run", VARIANT_RUNS, ids=["%s-%s" % (v[0], r) for v, r in VARIANT_RUNS])
def test_variant_at_regime(solver, var, run):
    """American P and explicit pair, dividends, put EU / AM, the fp32 state on the ring and on paired strips.  The put rows carry
    bc_rate = -r_d, hr0 = r_d / 2 and b2 = -r_d K / 2; at R2 and R3 the reference's put field exceeds K somewhere: the
    negative-rate edge data are in play."""
    name, m1, m2, N, tuning, want, absent, kw = var
    n = 4
    if run in R.RATE:
        w, a = _named(want, absent, run)
        _, Uo = _run(solver, "%s %s" % (name, run), tuning, w, a, m1, m2, N, n, *R.RATE[run], (M0,) * n, **kw)
        if kw.get("put") and run in ("R2", "R3"):
            assert (Uo.max(axis=1) > np.array(_inputs(m1, m2, n, True)[0])).all()
    else:
        _run(solver, "%s models %s" % (name, run), tuning, want, absent, m1, m2, N, n, *R.MODEL_RATES, _models(n, int(run[1:])), **kw)


# ---- d. team kernel and resident sweep x rates ----------------------------------------------------------------------------
TEAM_RATES = [(TEAM[0], rid, put) for rid in ("R0", "R1", "R2", "R6") for put in (False, True)] + [(TEAM[1], "R0", False), (TEAM[1], "R1", False)]


@pytest.mark.parametrize("team,rid,put", TEAM_RATES, ids=["%s-%s-%s" % (t[0], r, "put" if p else "call") for t, r, p in TEAM_RATES])
def test_team_kernel_at_rate(solver, team, rid, put):
    """R1 with put data is bc_rate = -r_d = 0 beside q != 0: the branch that skips the per-step exp (unit_e) with put boundary
    data.  At R0 q = 0: the library keeps the team kernel off, as it keeps the strips off, and the streaming kernels answer."""
    _need_256(solver)
    name, m1, m2, N, n, variant, kernel = team
    want, absent = ([], ["hadi_team_kernel", "strip"]) if rid in R.Q_ZERO else ([kernel], [])
    _run(solver, "%s %s %s" % (name, rid, "put" if put else "call"), {"team_launch": 1}, want, absent, m1, m2, N, n, *R.RATE[rid], (M0,) * n,
         variant=variant, put=put)


RESIDENT_RATES = [(rid, False) for rid in ("R1", "R2", "R3", "R5", "R6")] + [("R1", True), ("R2", True)]


@pytest.mark.parametrize("rid,put", RESIDENT_RATES, ids=["%s-%s" % (r, "put" if p else "call") for r, p in RESIDENT_RATES])
def test_resident_sweep_at_rate(solver, rid, put):
    """(R4 and q = 0 are in test_gpu_resident.py::INPUTS_C.)"""
    _need_256(solver)
    _resident_pair(solver, "resident %s %s" % (rid, "put" if put else "call"), 4, *R.RATE[rid], (M0,) * RES[2], put=put)


# ---- e. schemes -------------------------------------------------------------------------------------------------------------
SCHEME_PATHS = [("ring", 128, 64, _st()), ("strips", 300, 80, _st(strip=1)), ("small_sch_50x25", 50, 25, {"small_sch": 1}),
                ("small_sch_100x20", 100, 20, {"small_sch": 1})]
SCHEME_RUNS = RATE_IDS + ["c%d" % c for c in _rotations(4)]


@pytest.mark.parametrize("run", SCHEME_RUNS)
@pytest.mark.parametrize("scheme,theta,name", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning", SCHEME_PATHS, ids=[p[0] for p in SCHEME_PATHS])
def test_scheme_at_regime(solver, path, m1, m2, tuning, scheme, theta, name, run):
    """CS / MCS / HV against tests/scheme_ref.py (the oracle for CS); at R0 and R7 forced strips fall back to the shared ring."""
    if path == "ring":
        want, absent = ["hadi_pass_a", ",%s>" % name], ["strip", SMALL_SCH]
    elif path == "strips" and run in R.Q_ZERO:
        want, absent = ["hadi_pass_a", "<8,1,", ",%s>" % name], ["strip", SMALL_SCH]  # (hadi_pass_a<8,1,..,CS> / hadi_pass_a_sch<8,1,..>)
    elif path == "strips":
        want, absent = ["hadi_pass_a_strip%s<8,EU,double,1,%s>" % ("" if name == "CS" else "_sch", name)], [SMALL_SCH]
    else:
        want, absent = [SMALL_SCH + "%d,%s>" % (1 if m1 <= 64 else 2, name)], []
    n, N = 4, 3
    rates, models = (R.RATE[run], (M0,) * n) if run in R.RATE else (R.MODEL_RATES, _models(n, int(run[1:])))
    _run(solver, "%s %s %s" % (name, path, run), tuning, want, absent, m1, m2, N, n, *rates, models, scheme=scheme, theta=theta)


# ---- f. launchers and Greeks ------------------------------------------------------------------------------------------------
LAUNCH_REGIMES = [(rid, R.RATE[rid], M0) for rid in ("R1", "R2", "R4")] + [(mid, R.MODEL_RATES, R.MODEL[mid]) for mid in ("M4", "M6", "M7")]
LAUNCH_SHAPES = [("small_50x25", 50, 25, {"small_seq": 1}, ["hadi_small_seq_kernel<1>"], ["hadi_small_"]),
                 ("ring_128x64", 128, 64, _st(), ["hadi_pass_a<2,1,", ",EU>"], ["hadi_pass_a<2,1,", "AM"])]


@pytest.mark.parametrize("rid,rates,model", LAUNCH_REGIMES, ids=[r[0] for r in LAUNCH_REGIMES])
@pytest.mark.parametrize("name,m1,m2,tuning,want_eu,want_amdiv", LAUNCH_SHAPES, ids=[s[0] for s in LAUNCH_SHAPES])
def test_launchers_at_regime(solver, name, m1, m2, tuning, want_eu, want_amdiv, rid, rates, model):
    """compute_base_prices, compute_jacobian and compute_jacobian_american_dividends against Cm.OracleSolver: prices 1e-9,
    J 2e-4.  M6 (kappa = 0) is in: the oracle's forward differences are well-defined there -- finite, the kappa column the
    one-sided derivative at 0 (0.09 .. 0.22 on these grids), the eta column exactly 0 since eta enters through kappa (eta - v)
    only -- and both facts are asserted on the reference."""
    n0, N = 3, 10
    strikes, grids, U0, V0 = _inputs(m1, m2, n0)
    total = (m1 + 1) * (m2 + 1)
    args = (Cm.S_0, V0, Cm.T, *rates, *model, m1, m2, total, N, Cm.THETA, Cm.T / N, n0, grids)
    div = H.Dividends(*Cm.DIVS)
    ws = H.DOWorkspace(n0, total)
    ws.U[...] = U0
    with _tuned(solver, tuning):
        prices = solver.compute_base_prices(*args, ws)
        dp = solver.describe_last_sweep()
        J, base = solver.compute_jacobian(*args, U0)
        d = solver.describe_last_sweep()
        Ja, basea = solver.compute_jacobian_american_dividends(*args, U0, div)
        da = solver.describe_last_sweep()
    _has(dp, want_eu)
    _has(d, want_eu)
    _has(da, want_amdiv)
    orc = Cm.OracleSolver()
    wso = H.DOWorkspace(n0, total)
    wso.U[...] = U0
    po = orc.compute_base_prices(*args, wso)
    Jo, bo = orc.compute_jacobian(*args, U0)
    Jao, bao = orc.compute_jacobian_american_dividends(*args, U0, div)
    for x in (po, Jo, bo, Jao, bao):
        assert np.isfinite(x).all()
    live = [0, 2, 3, 4] if rid == "M6" else [0, 1, 2, 3, 4]  # (columns kappa, eta, sigma, rho, v0: every one a real derivative)
    assert (np.abs(Jo).max(axis=0)[live] > 1e-6).all() and (np.abs(Jao).max(axis=0)[live] > 1e-6).all(), (Jo, Jao)
    assert rid != "M6" or (Jo[:, 1] == 0.0).all()
    # the regime moved the reference: every option's price, European and American with dividends, by >= 1e-6 of itself from
    # the canonical-parameter one (rate regimes: canonical rates; model regimes: M0 at the same rates)
    canon = (Cm.S_0, V0, Cm.T, *(R.CANONICAL_RATES if model == M0 else rates), *M0) + args[9:]
    pc, bac = orc.compute_base_prices(*canon, wso), orc.compute_jacobian_american_dividends(*canon, U0, div)[1]
    moved = min((np.abs(po - pc) / np.abs(pc)).min(), (np.abs(bao - bac) / np.abs(bac)).min())
    assert moved >= 1e-6, moved
    ep, eb, eJ = np.abs(prices - po).max(), max(np.abs(base - bo).max(), np.abs(basea - bao).max()), max(np.abs(J - Jo).max(), np.abs(Ja - Jao).max())
    print("%s %s: prices %.3e, base %.3e, J %.3e" % (name, rid, ep, eb, eJ))
    assert ep < 1e-9 and eb < 1e-9, (ep, eb)
    assert eJ < 2e-4, eJ


GREEK_REGIMES = [(rid, R.RATE[rid], M0) for rid in ("R0", "R2", "R6")] + [(mid, R.MODEL_RATES, R.MODEL[mid]) for mid in ("M1", "M3")]
GREEK_SHAPES = [("ring_128x64", 128, 64, _st(), "hadi_pass_a<2,1,"), ("strips_300x80", 300, 80, _st(strip=1), "hadi_pass_a_strip<8,")]
GREEK_KINDS = [(H.EU, False), (H.EU, True), (H.AM, False), (H.AM, True)]


def _greeks(sv, tuning, m1, m2, N, n, rates, model, variant, put, k=0):
    strikes, grids, U0, divs = _scaled_inputs(m1, m2, n, put, k)
    with _tuned(sv, tuning):
        out = sv.compute_greeks(m1, m2, N, Cm.T / N, Cm.THETA, *rates, *model, grids, U0.copy(), Cm.S_0 * 2.0 ** k, _v0(m2), variant=variant,
                                option_type=H.PUT if put else H.CALL, strikes=list(strikes) if put else None, ladder=True)
        d = sv.describe_last_sweep()
    return out[0], out[1], d


@pytest.mark.parametrize("rid,rates,model", GREEK_REGIMES, ids=[r[0] for r in GREEK_REGIMES])
@pytest.mark.parametrize("variant,put", GREEK_KINDS, ids=["EU_call", "EU_put", "AM_call", "AM_put"])
@pytest.mark.parametrize("name,m1,m2,tuning,kernel", GREEK_SHAPES, ids=[s[0] for s in GREEK_SHAPES])
def test_greeks_and_ladder_at_regime(solver, name, m1, m2, tuning, kernel, variant, put, rid, rates, model):
    """compute_greeks with the ladder against tests/greeks_ref.py on the oracle's field, at the propagated bound of
    test_gpu_greeks.py.  The theta column is where bc_rate, half_rd and hr0 show."""
    n, N = 2, 4
    strikes, grids, U0, V0 = _inputs(m1, m2, n, put)
    greeks, lad, d = _greeks(solver, tuning, m1, m2, N, n, rates, model, variant, put)
    _has(d, *_named([kernel], [], rid))
    worst = 0.0
    for k in range(n):
        p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, *rates, *model, OV[variant], option_type=O.PUT if put else O.CALL,
                          strikes=[strikes[k]] if put else None)
        g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
        b, U, lam = G.boundary_vector(p, *g, U0[k], U0[k] if variant == H.AM else None)
        assert np.isfinite(U).all()
        pc = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, *(R.CANONICAL_RATES if model == M0 else rates), *M0, OV[variant],
                           option_type=O.PUT if put else O.CALL, strikes=[strikes[k]] if put else None)
        Uc = O.solve(pc, *g, U0[k], U0[k] if variant == H.AM else None)[0]
        assert np.abs(U - Uc).max() >= 1e-6 * np.abs(Uc).max()  # (the regime moved the reference)
        j0, i0 = G.find_node(g[1], V0), G.find_node(g[0], Cm.S_0)
        assert i0 >= 0 and j0 >= 0
        ref = G.ladder(p, *g, U, lam, j0, b)
        bound = G.propagated_bound(p, g[0], g[1], j0, np.abs(U).max())
        r, where = G.worst_ratio(lad[k], ref, bound)
        assert r <= 1.0, "instance %d node %d column %s: got %.17g ref %.17g bound %.3e" % (
            k, where[0], G.NAMES[where[1]], lad[k][where], ref[where], bound[where])
        assert np.array_equal(greeks[k], lad[k, i0])
        worst = max(worst, r)
    print("%s %s %s: Greeks ladder, worst |diff| / bound %.3e" % (name, rid, "put" if put else "call", worst))


# ---- g. spot scale (reference-free) -------------------------------------------------------------------------------------------
EU_CALL, DIV_PUT, AM_PUT, AMDIV_CALL = (H.EU, False), (H.DIV, True), (H.AM, True), (H.AM_DIV, False)
ALL4 = (EU_CALL, DIV_PUT, AM_PUT, AMDIV_CALL)
EUR = (EU_CALL, DIV_PUT)  # (the sequential LDS kernels: European and dividend sweeps only)
# The kernel every variant of a row must describe: {t} is EU for the European and dividend sweeps and, for the American ones,
# the last column -- AM-P where the sweep runs in the P representation (american_p = 1, a payoff that depends on s alone), AM
# on the LDS kernel and on the sequential passes, which keep the explicit (U, lambda_bar) pair (hadi_api.hip, `amp`).  "row" /
# "col": looked for in the row-pass / column-pass half of the description only (both halves carry a tag).
#               class                   row of FAMILIES          variants  where   the description names                                   and not        American tag
SCALE_ROWS = [("small block",          "small_eu",              ALL4,     "all",  ["hadi_small_kernel<1,", ",{t}>"],                        [],            "AM"),
              ("small seq",            "small_seq",             EUR,      "all",  ["hadi_small_seq_kernel<1>"],                             [],            None),
              ("seq2",                 "small_seq2_n5",         EUR,      "all",  ["hadi_small_seq2_kernel<1>"],                            [],            None),
              ("ring b1",              "ring_b1",               ALL4,     "row",  ["hadi_pass_a<1,1,", ",{t}>"],                            ["strip"],     "AM-P"),
              ("ring b4",              "ring_b4",               ALL4,     "row",  ["hadi_pass_a<4,1,", ",{t}>"],                            ["strip"],     "AM-P"),
              ("ring b8",              "ring_b8",               ALL4,     "row",  ["hadi_pass_a<8,1,", ",{t}>"],                            ["strip"],     "AM-P"),
              ("ring two-wavefronts",  "ring_two_wavefronts",   ALL4,     "row",  ["hadi_pass_a<8,2,", ",{t}>"],                            ["strip"],     "AM-P"),
              ("strips b8",            "strips_b8",             ALL4,     "row",  ["hadi_pass_a_strip<8,{t}>"],                             [],            "AM-P"),
              ("pairs",                "pairs",                 ALL4,     "row",  ["hadi_pass_a_pairs<{t}>"],                               [],            "AM-P"),
              ("paired strips",        "paired_strips_rs_tab",  ALL4,     "row",  ["hadi_pass_a_strip<8,{t},double,2>", "paired strips"],   [],            "AM-P"),
              ("pass_b1",              "pass_b1",               ALL4,     "col",  ["hadi_pass_b1<16,{t}>"],                                 [],            "AM-P"),
              ("pass_b_seq",           "pass_b_seq",            ALL4,     "col",  ["hadi_pass_b_seq<{t}>"],                                 [],            "AM"),
              ("pass_a_seq",           "pass_a_seq",            ALL4,     "row",  ["hadi_pass_a_seq<{t}>"],                                 [],            "AM")]
FAMILY = {f[0]: f for f in FAMILIES}
SCALE_CASES = [(r, v) for r in SCALE_ROWS for v in r[2]]
VNAME = {EU_CALL: "EU_call", DIV_PUT: "DIV_put", AM_PUT: "AM_put", AMDIV_CALL: "AMDIV_call"}
COLUMN = "; column pass "


def _names(row, v):
    """(the names the description of this row must hold for variant v, the names it must not, the half they are looked for in)"""
    _, _, _, where, want, absent, am_tag = row
    tag = am_tag if v[0] in (H.AM, H.AM_DIV) else "EU"
    other = sorted({"EU", "AM", "AM-P"} - {tag})
    want = [w.format(t=tag) for w in want]
    absent = list(absent) + [w.format(t=o) for w in row[4] if "{t}" in w for o in other]
    return want, absent, where


def _half(d, where):
    assert where == "all" or COLUMN in d, d
    return d if where == "all" else d.split(COLUMN)[0] if where == "row" else d.split(COLUMN)[1]


def _scaling(sv, name, tuning, want, m1, m2, N, n, variant, put, rows=None, absent=(), where="all"):
    """U(2^k inputs) == 2^k U and lambda_bar likewise, np.array_equal, for k = 9, -7, 30, -30; every scaled field against the
    oracle SOLVED ON THE SCALED INPUTS at 1e-10.  The scaled call must describe the kernels of the unscaled one."""
    rates, models = R.MODEL_RATES, (M0,) * n
    U, lam, d = _sweep(sv, tuning, m1, m2, N, n, *rates, models, variant=variant, put=put)
    _has(_half(d, where), want, absent)
    assert lam is None or np.abs(lam).max() > 0
    sel = slice(None) if rows is None else list(rows)
    same = True
    for k in R.SCALE_POWERS:
        Us, ls, ds = _sweep(sv, tuning, m1, m2, N, n, *rates, models, variant=variant, put=put, k=k)
        assert ds == d, (ds, d)
        Uo, lo = _reference(m1, m2, N, n, *rates, models, variant=variant, put=put, k=k, rows=rows)
        _check("%s 2^%d" % (name, k), Us[sel], None if ls is None else ls[sel], Uo, lo)
        same = same and np.array_equal(Us, U * 2.0 ** k) and (lam is None or np.array_equal(ls, lam * 2.0 ** k))
        assert same, "%s: the field of the inputs times 2^%d is not 2^%d times the field, bit for bit (max relative gap %.3e)" % (
            name, k, k, (np.abs(Us - U * 2.0 ** k) / np.abs(Us).max()).max())
    print("%s: scaling identity holds bit for bit at k = %s" % (name, (R.SCALE_POWERS,)))


@pytest.mark.parametrize("row,v", SCALE_CASES, ids=["%s-%s" % (r[1], VNAME[v]) for r, v in SCALE_CASES])
def test_spot_scaling_is_exact(solver, row, v):
    """Every variant asserts ITS kernel of the row's family (_names): a dividend, put or American sweep that left the strips, the
    pairs or the single-buffer column pass for another kernel would fail here, not pass under the family's name."""
    name, m1, m2, n, tuning, fam_want, _, kw = FAMILY[row[1]]
    variant, put = v
    N = 10 if variant in (H.DIV, H.AM_DIV) else 3  # (N = 10: all four dividend dates land on a step)
    want, absent, where = _names(row, v)
    if v == EU_CALL:
        want = want + [w for w in fam_want if w not in want]  # (the European call also names what the family's own row names)
    _scaling(solver, "%s %s" % (row[0], VNAME[v]), tuning, want, m1, m2, N, n, variant, put, absent=absent, where=where)


@pytest.mark.parametrize("v", [EU_CALL, DIV_PUT], ids=["EU_call", "DIV_put"])
def test_spot_scaling_is_exact_on_the_team_kernel(solver, v):
    _need_256(solver)
    _, m1, m2, _, n, _, kernel = TEAM[1]
    _scaling(solver, "team %s" % VNAME[v], {"team_launch": 1}, [kernel], m1, m2, 10, n, *v)


@pytest.mark.parametrize("put", [False, True], ids=["EU_call", "EU_put"])
def test_spot_scaling_is_exact_on_the_resident_sweep(solver, put):
    """256 instances; the fixed subset against the oracle, every instance in the identity."""
    _need_256(solver)
    m1, m2, n = RES
    _scaling(solver, "resident %s" % ("put" if put else "call"), {"resident_sweep": 1}, [RESIDENT], m1, m2, 4, n, H.EU, put, rows=SUBSET)


POWER = np.array([1, 0, -1, 1, 1, 0, 1, 1])  # price, delta, gamma, dv, dvv, dsv, theta, lambda: the power of 2^k each column takes


@pytest.mark.parametrize("variant,put", GREEK_KINDS, ids=["EU_call", "EU_put", "AM_call", "AM_put"])
@pytest.mark.parametrize("name,m1,m2,tuning,kernel", GREEK_SHAPES, ids=[s[0] for s in GREEK_SHAPES])
def test_greeks_scale_column_by_column(solver, name, m1, m2, tuning, kernel, variant, put):
    """k = 9 and -7 only: the 1e-10 node search of S_0 is absolute (hadi.h), so a spot axis times 2^-30 has no meaningful node
    search -- documented behaviour.  price, dv, dvv, theta, lambda by 2^k; delta and dsv by 1; gamma by 2^-k; bit for bit."""
    n, N = 2, 4
    g0, l0, d = _greeks(solver, tuning, m1, m2, N, n, R.MODEL_RATES, M0, variant, put)
    _has(d, [kernel])
    assert np.isfinite(l0).all() and (variant != H.AM or np.abs(l0[..., G.LAMBDA]).max() > 0)
    for k in (9, -7):
        gs, ls, ds = _greeks(solver, tuning, m1, m2, N, n, R.MODEL_RATES, M0, variant, put, k=k)
        assert ds == d
        f = 2.0 ** (k * POWER)
        bad = [G.NAMES[c] for c in range(8) if not (np.array_equal(ls[..., c], l0[..., c] * f[c]) and np.array_equal(gs[:, c], g0[:, c] * f[c]))]
        assert not bad, (name, k, bad)
    print("%s: every Greeks column scales exactly at k = 9, -7" % name)


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def test_every_row_meets_every_regime():
    """The tables above against FAMILIES / VARIANTS / SCHEMES of test_gpu_mixed_vgrids.py: a row added there later is in every
    rate regime and on every model here, or this fails."""
    rates, models = set(R.RATE), {m[1:] for m in R.MODELS}
    assert len(rates) == 8 and len(models) == 9 and RATE_IDS == sorted(rates)
    fam = {f[0] for f in FAMILIES}
    assert len(fam) == len(FAMILIES)
    for f in FAMILIES:
        seen = {m for ff, c in FAMILY_MODELS if ff[0] == f[0] for m in _models(f[3], c)}
        assert seen == models, f[0]
        if any("strip" in w or "pairs" in w for w in f[5]):
            w, a = _off_strips(f[5], f[6])
            assert w != f[5] and "strip" in a and all("strip" not in x for x in w), f[0]
    for v in VARIANTS:
        runs = {r for vv, r in VARIANT_RUNS if vv[0] == v[0]}
        assert rates <= runs, v[0]
        assert {m for r in runs - rates for m in _models(4, int(r[1:]))} == models, v[0]
    assert set(SCHEME_RUNS) >= rates and {m for r in SCHEME_RUNS if r not in rates for m in _models(4, int(r[1:]))} == models
    assert [s[2] for s in SCHEMES] == ["CS", "MCS", "HV"]
    for t in TEAM:
        assert {m for tt, c in TEAM_MODELS if tt[0] == t[0] for m in _models(t[4], c)} == models
    assert {r[1] for r, _ in SCALE_CASES} <= fam
    # every family class of the scaling list is there, and R6 keeps a non-zero q in fp64 (so the host keeps the strips)
    assert len({r[0] for r, _ in SCALE_CASES}) == 13 and R.RATE["R6"][0] - R.RATE["R6"][1] != 0.0
    for r, v in SCALE_CASES:  # every scaling case names a kernel of its family, and the tagged ones exclude the other tags
        want, absent, where = _names(r, v)
        assert want and all("{" not in w for w in want + absent) and where in ("all", "row", "col"), (r[0], v)
        assert r[6] is None or absent, (r[0], v)
        if v == EU_CALL:  # the European name is the one the family's own row asserts
            assert any(w in f or f in w for w in want for f in FAMILY[r[1]][5]), r[0]
