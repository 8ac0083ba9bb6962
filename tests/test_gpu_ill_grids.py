"""Every kernel family on ILL-conditioned grids, judged against binary128 (tests/ill_grids.py).

The rest of the suite builds its batches with Cm.well_conditioned_strikes / Cm.v0_for and asserts the 30x rule before it compares
anything; callers do not: hadi_make_grid inserts S_0 into a fixed sinh grid, the v-grid is rebuilt on the device for V_0 + eps and
for every V_0_i an LM iteration tries.  Here every instance carries an interval 1e4 or 1e6 times shorter than its neighbour,
PLACED where the kernels change what they do: on the s-axis at the first and the last interval, between two lanes, inside a lane,
astride the two wavefronts of a row, at the strike and at 100; on the v-axis at the first interval, at V_0 = 0.04, at rows 32 | 33
(the column-chunk edge, HADI_LC = 33), at a strip edge of the row pass (the height is read from describe_last_sweep()) and in the
last two intervals.  Turn 0 and turn 1 give every position both ratios.

Judged per instance by ill_grids.judge -- finite; sanity cap 1e-4 / 1e-3 against the fp64 oracle; inside the well-conditioned band
(1e-10 / 1e-8) nothing further; otherwise |U - U_x| / max|U_x| < max(30 yard, 1e-11) against oracle.solve_xp, `yard` the fp64
oracle's own distance from binary128 over the instance and its two siblings.  None of these numbers was fitted to a run.  MCS and
HV have no exact reference: finite and the cap against tests/scheme_ref.py, the difference printed.  The fp32 state is out of
scope (it has its own yardstick, tests/test_gpu_regressions.py).

No new launch configuration: FAMILIES, VARIANTS, SCHEMES, SMALL_SCH and RESIDENT of tests/test_gpu_mixed_vgrids.py, the team rows
of tests/test_gpu_regimes.py.  Every case asserts from describe_last_sweep() which kernel ran and prints e_h, e_o, yard and
e_h / yard of every adjudicated instance."""
import re

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from oracle import oracle as O

import common as Cm
import greeks_ref as G
import ill_grids as I
import samples_ref as SR
import scheme_ref as S
from test_gpu_mixed_vgrids import FAMILIES, OV, RESIDENT, SCHEMES, SMALL_SCH, VARIANTS, _has, _st, _tuned
from test_gpu_regimes import TEAM

pytestmark = pytest.mark.gpu

R_F = 0.01
AXES_TURNS = [("s", 0), ("s", 1), ("v", 0), ("v", 1)]
AT_IDS = ["%s%d" % at for at in AXES_TURNS]


def gridviews(insts, put=False):
    """(strikes, GridViewsBatch, U0) of a batch of ill_grids instances: the oracle's builder made the arrays."""
    ks, vs, vv, ds, dv, U0 = I.arrays(insts, put)
    g = object.__new__(H.GridViewsBatch)
    g.m1, g.m2, g.n = insts[0].m1, insts[0].m2, len(insts)
    g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v = vs, vv, ds, dv
    return [float(k) for k in ks], g, U0


def _sweep(sv, tuning, insts, c, scheme=0):
    """One DO_timestepping of the batch under `tuning` -> (U_T, lambda_bar_T or None, description, team state)."""
    strikes, grids, U0 = gridviews(insts, c.put)
    m1, m2 = grids.m1, grids.m2
    variant = {v: k for k, v in OV.items()}[c.variant]
    american = variant in (H.AM, H.AM_DIV)
    U, lam = U0.copy(), (np.zeros_like(U0) if american else None)
    with _tuned(sv, tuning):
        sv.DO_timestepping(m1, m2, c.N, Cm.T / c.N, c.theta, Cm.R_D, c.r_f, *c.model, grids, U, variant=variant,
                           U_0=U0.copy() if american else None, lambda_bar=lam,
                           dividends=H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None, scheme=scheme,
                           option_type=H.PUT if c.put else H.CALL, strikes=strikes if c.put else None)
        d = sv.describe_last_sweep()
        state = sv.get_tuning("team_launch")
    return U, lam, d, state


def _strip_rows(d):
    """Height of the row pass's strips as the description states it; None where the row pass runs no strips."""
    m = re.search(r"strips of (\d+) rows", d)
    return int(m.group(1)) if m else None


def _batch(sv, tuning, m1, m2, axis, turn, c, scheme=0, fixed_n=None, odd=False):
    """The batch of the case, admitted (ill_grids.admit): one instance per position of the axis (one more where `odd` asks for an
    odd count), or fixed_n.  On the v-axis the strip height comes from the description of a sweep of a batch of the same size
    under the same tuning; the real sweep must state the same height (asserted by the caller through _strip_rows)."""
    def count(npos):
        return fixed_n or (npos | 1 if odd else npos)

    if axis != "v":
        return I.admit(c, I.batch(m1, m2, count(len(I.s_positions(m1, 100.0))), axis, turn)), None
    nv = len(I.v_positions(m2))
    _, _, d, _ = _sweep(sv, tuning, I.batch(m1, m2, count(nv + 1), "s", 0), c, scheme)
    rs = _strip_rows(d)
    if len(I.v_positions(m2, rs)) == nv:   # no strips, or no strip edge that is a position of its own
        rs = None
    return I.admit(c, I.batch(m1, m2, count(nv + (rs is not None)), "v", turn, rs)), rs


def _judge(name, c, insts, U, lam):
    ok, verdicts = I.judge_batch(name, c, insts, U, lam)
    assert ok, [(k, I.describe(insts[k]), v) for k, v in enumerate(verdicts) if not v["ok"]]
    return verdicts


def _cap_only(name, c, insts, U, which):
    """MCS / HV: finite and the sanity cap against tests/scheme_ref.py; the difference is printed, nothing else is claimed."""
    ks, vs, vv, ds, dv, U0 = I.arrays(insts)
    for k, inst in enumerate(insts):
        Uo = S.solve_one(I.params(c, inst), vs[k], vv[k], ds[k], dv[k], U0[k], which)
        assert np.isfinite(U[k]).all() and np.isfinite(Uo).all(), (name, k)
        d = np.abs(U[k] - Uo).max() / np.abs(Uo).max()
        print("  %s #%d %s: |U - U_ref| %.2e of max|U_ref|" % (name, k, I.describe(inst), d))
        assert d <= I.CAP_U, (name, k, d)


def _run_case(sv, name, tuning, want, absent, m1, m2, axis, turn, c, scheme=0, fixed_n=None, odd=False):
    insts, rs = _batch(sv, tuning, m1, m2, axis, turn, c, scheme, fixed_n, odd)
    U, lam, d, state = _sweep(sv, tuning, insts, c, scheme)
    _has(d, want, absent)
    assert tuning.get("team_launch") != 1 or state == 1, (d, state)
    assert rs is None or _strip_rows(d) == rs, (rs, d)
    label = "%s %s turn %d" % (name, axis, turn)
    if scheme in (H.SCHEME_MCS, H.SCHEME_HV):
        _cap_only(label, c, insts, U, S.MCS if scheme == H.SCHEME_MCS else S.HV)
        return None
    return _judge(label, c, insts, U, lam)


# ---- a. Douglas, every family -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
@pytest.mark.parametrize("name,m1,m2,n,tuning,want,absent,kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_douglas_family(solver, name, m1, m2, n, tuning, want, absent, kw, axis, turn):
    """One instance per position of the axis (an odd number of them where the family's own row has an odd one: the tail of
    the two-instances-per-wavefront kernel)."""
    c = I.cfg(3, r_f=R_F, variant=OV[kw.get("variant", H.EU)])
    _run_case(solver, name, tuning, want, absent, m1, m2, axis, turn, c, odd=bool(n % 2))


# ---- b. variants --------------------------------------------------------------------------------------------------------
def _row(name):
    return next(v for v in VARIANTS if v[0] == name)


def _variant_rows():
    """AM in the P representation and on the explicit pair, DIV, AM_DIV and put data on an LDS-resident row, a ring row, a strip
    row and the two-wavefront row.  Ring and strip rows: VARIANTS; the other two: the FAMILIES rows small_eu and
    ring_two_wavefronts with the variant's name in the kernel's."""
    out = []
    lds = ("lds", 50, 25, {"small_seq": 0}, "hadi_small_kernel<1,")
    two = ("two_wavefronts", 600, 40, _st(), "hadi_pass_a<8,2,")
    for tag, m1, m2, tuning, k in (lds, two):
        out += [("%s_am_p" % tag, m1, m2, 3, dict(tuning, american_p=1), [k, "AM"], [], dict(variant=H.AM)),
                ("%s_am_pair" % tag, m1, m2, 3, dict(tuning, american_p=0), [k, ",AM>"], ["AM-P"], dict(variant=H.AM)),
                ("%s_div" % tag, m1, m2, 10, tuning, [k], ["AM"], dict(variant=H.DIV)),
                ("%s_am_div" % tag, m1, m2, 10, tuning, [k, "AM"], [], dict(variant=H.AM_DIV)),
                ("%s_put" % tag, m1, m2, 3, tuning, [k], ["AM"], dict(put=True))]
    out += [_row(x) for x in ("am_p_ring", "am_pair_ring", "am_div_ring", "am_p_strips", "am_pair_strips", "am_div_strips", "div_strips")]
    out += [("div_ring", 128, 64, 10, _st(), ["hadi_pass_a<2,1,", ",EU>"], ["strip"], dict(variant=H.DIV)),
            ("put_ring", 128, 64, 3, _st(), ["hadi_pass_a<2,1,", ",EU>"], ["strip"], dict(put=True)),
            ("put_strips", 300, 140, 3, _st(strip=1), ["hadi_pass_a_strip<8,EU>"], [], dict(put=True))]
    return out


VARIANT_ROWS = _variant_rows()


@pytest.mark.parametrize("axis,turn", [("s", 0), ("v", 1)], ids=["s0", "v1"])
@pytest.mark.parametrize("name,m1,m2,N,tuning,want,absent,kw", VARIANT_ROWS, ids=[v[0] for v in VARIANT_ROWS])
def test_variant(solver, name, m1, m2, N, tuning, want, absent, kw, axis, turn):
    """Field and lambda_bar both go through the rule (N = 10 with dividends: with fewer than five steps no dividend date meets
    the reference's dating rule)."""
    c = I.cfg(N, r_f=R_F, variant=OV[kw.get("variant", H.EU)], put=kw.get("put", False))
    _run_case(solver, name, tuning, want, absent, m1, m2, axis, turn, c)


# ---- c. predictor-corrector schemes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,turn", [("s", 0), ("v", 1)], ids=["s0", "v1"])
@pytest.mark.parametrize("scheme,theta,name", SCHEMES, ids=[s[2] for s in SCHEMES])
@pytest.mark.parametrize("path,m1,m2,tuning", [("ring", 128, 64, _st()), ("strips", 300, 80, _st(strip=1)), ("no_strips", 300, 80, _st(strip=0)),
                                               ("small_sch_b1", 50, 25, {"small_sch": 1}), ("small_sch_b2", 100, 20, {"small_sch": 1})],
                         ids=["ring", "strips", "strips_off", "small_sch_50x25", "small_sch_100x20"])
def test_scheme(solver, path, m1, m2, tuning, scheme, theta, name, axis, turn):
    """Craig-Sneyd by the rule on the streaming ring, on its strips, with the strips off and on hadi_small_sch_kernel; MCS and HV
    on the same paths, finite and under the cap."""
    if path in ("ring", "no_strips"):
        want, absent = ["hadi_pass_a", ",%s>" % name], ["strip", SMALL_SCH]
    elif path == "strips":
        want, absent = ["hadi_pass_a_strip%s<8,EU,double,1,%s>" % ("" if name == "CS" else "_sch", name)], [SMALL_SCH]
    else:
        want, absent = [SMALL_SCH + "%d,%s>" % (1 if m1 <= 64 else 2, name)], []
    c = I.cfg(3, theta=theta, r_f=0.007, scheme=1 if scheme == H.SCHEME_CRAIG_SNEYD else 0)
    _run_case(solver, "%s %s" % (name, path), tuning, want, absent, m1, m2, axis, turn, c, scheme=scheme)


# ---- d. one launch for the whole loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,turn", AXES_TURNS, ids=AT_IDS)
@pytest.mark.parametrize("team", TEAM, ids=[t[0] for t in TEAM])
def test_team_kernel(solver, team, axis, turn):
    """hadi_team_kernel on 300x140 with 3 instances (turns 0 and 3: six positions) and on 256x128 with dividends and 8."""
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the instance-resident launch needs the 256-CU device")
    name, m1, m2, N, n, variant, kernel = team
    c = I.cfg(N, r_f=R_F, variant=OV[variant])
    _run_case(solver, name, {"team_launch": 1}, [kernel], [], m1, m2, axis, turn * (3 if n == 3 else 1), c, fixed_n=n)


@pytest.mark.parametrize("axis", ["s", "v"])
def test_resident_sweep_256_instances(solver, axis):
    """hadi_sweep_resident<8> on 300x80 x 256, every instance ill-conditioned on the axis: the band against the oracle on 16
    threads, every instance outside it adjudicated, and the field against the same call on the streaming kernels at 1e-13."""
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("256 instances are one round of blocks on the 256-CU device only")
    m1, m2, n = 300, 80, 256
    c = I.cfg(3, r_f=R_F)
    insts, rs = _batch(solver, {"resident_sweep": 1}, m1, m2, axis, 0, c, fixed_n=n)
    U, _, d, _ = _sweep(solver, {"resident_sweep": 1}, insts, c)
    Us, _, ds, _ = _sweep(solver, {"resident_sweep": 0}, insts, c)
    _has(d, ["both passes of every step in one launch: " + RESIDENT])
    _has(ds, [], [RESIDENT])
    assert rs is None or _strip_rows(d) == rs, (rs, d)
    rel = np.abs(U - Us).max() / np.abs(Us).max()
    print("resident vs streaming, max |dU| / max |U| = %.3e" % rel)
    assert rel <= 1e-13
    _judge("resident 300x80 x 256 %s" % axis, c, insts, U, None)


# ---- e. launchers and the device-side rebuild -----------------------------------------------------------------------------
EPS = 1e-6
BUMPS = ("kappa", "eta", "sigma", "rho", "v0")  # the columns of J


def _launcher_instances(m1, m2, sR):
    """Four options on ONE strike (the launchers take one scalar S_0, which must sit beside a raw node of every instance's
    s-grid): S_0 h / sR above the lower node of the raw interval that holds 100; V_0_i beside the raw v-node below 0.04 -- above it
    and below it at 1e4, above it at the other ratio of ill_grids.BOTH_RATIOS -- and V_0 = v_j - eps / 2, whose bump V_0 + eps
    crosses the raw node, so that the sixth group's grid has another node order than the base grid."""
    K = Cm.well_conditioned_strikes(m1, 1)[0]
    si = next(t for name, kind, t in I.s_positions(m1, K) if name == "holds 100")
    raw_s, raw_v = I.raw_s(m1, K), I.raw_v(m2)
    j = next(t for name, kind, t in I.v_positions(m2) if name.startswith("holds V_0"))
    sR = I.fit_ratio(raw_s[si + 1] - raw_s[si], sR)
    other = 1e6 if sR == 1e4 else 1e4
    h, hb = raw_v[j + 1] - raw_v[j], raw_v[j] - raw_v[j - 1]
    specs = [("above the node", j, "lower", I.fit_ratio(h, 1e4)), ("below the node", j - 1, "upper", I.fit_ratio(hb, 1e4)),
             ("above the node", j, "lower", I.fit_ratio(h, other)), ("bump crosses the node", j - 1, "upper", hb / (EPS / 2))]
    insts = tuple(I.Inst(m1, m2, float(K), si, sR, "lower", vj, vR, side, None, "holds 100", name) for name, vj, side, vR in specs)
    cross = I.grids(insts[3])[5]
    assert cross < raw_v[j] < cross + EPS and raw_v[j] - cross >= I.MIN_INTERVAL
    return insts


def _price_at(U, vs, vv, s0, v0, m1):
    i, j = I.find_all(vs, s0), I.find_all(vv, v0)
    assert len(i) == 1 and len(j) == 1, (i, j)
    return float(U[int(i[0]) + int(j[0]) * (m1 + 1)])


def _exact_prices(c, inst):
    """(base, the five bumped prices, max|U_x|) through binary128: the base grid for the four model bumps, the host-rebuilt grid
    of V_0 + eps for the fifth."""
    vs, vv, ds, dv, s0, v0 = I.grids(inst)
    Ux = I.exact(c, inst)[0]
    base = _price_at(Ux, vs, vv, s0, v0, inst.m1)
    rho, sigma, kappa, eta = c.model
    out = []
    for model in ((rho, sigma, kappa + EPS, eta), (rho, sigma, kappa, eta + EPS), (rho, sigma + EPS, kappa, eta), (rho + EPS, sigma, kappa, eta)):
        out.append(_price_at(I.exact(c._replace(model=model), inst)[0], vs, vv, s0, v0, inst.m1))
    vv6, dv6 = O.rebuild_variance(inst.m2, v0 + EPS)
    U0 = I.payoff(inst, vs, c.put)
    U6, _ = O.solve_xp(I.params(c, inst), vs, vv6, ds, dv6, U0, U0)
    out.append(_price_at(U6, vs, vv6, s0, v0 + EPS, inst.m1))
    return base, out, float(np.abs(Ux).max())


def _oracle_prices(c, inst):
    """(base, the five bumped prices base + eps J_g, max|U_ref|) of the fp64 oracle's launchers."""
    vs, vv, ds, dv, s0, v0 = I.grids(inst)
    g = tuple(np.ascontiguousarray(x[None, :]) for x in (vs, vv, ds, dv))
    U0 = I.payoff(inst, vs, c.put)[None, :]
    p = I.params(c, inst)
    po, Uo = O.base_prices(p, s0, v0, *g, U0, U0)
    Jo, bo = O.jacobian(p, s0, v0, *g, U0, eps=EPS)
    return float(po[0]), float(bo[0]), [float(bo[0] + EPS * Jo[0, q]) for q in range(5)], Jo[0], float(np.abs(Uo).max())


def _admitted_launcher_instances(c, m1, m2, sR):
    """The four options at the largest s-ratio <= sR (powers of ten) at which the two references agree within 1 / 31 of the sanity
    cap on every instance's field (ill_grids.admit; it may lower a V_0_i's own ratio) AND on all six prices of every instance:
    an American sweep with dividends can turn a parameter bump of 1e-6 into a different exercise boundary on such a grid -- the
    oracle's own J then holds entries of 1e8 and more, in binary128 as in fp64 -- and the cap must not be tripped by the reference
    alone.  Decided by the references, before the device runs; the ratio used is printed."""
    from multiprocessing.pool import ThreadPool
    while True:
        insts = _launcher_instances(m1, m2, sR)
        adm = I.admit(c, insts)
        if all(a.sR == b.sR for a, b in zip(adm, insts)) and adm[3] == insts[3]:
            with ThreadPool(len(adm)) as pool:
                ref = pool.map(lambda i: (_oracle_prices(c, i), _exact_prices(c, i)), adm)
            worst = max(max(abs(a - b) for a, b in zip([o[1]] + o[2], [x[0]] + x[1])) / x[2] for o, x in ref)
            if np.isfinite(worst) and worst <= I.CAP_U / 31:
                print("launchers %dx%d: s-ratio %.0e, references agree on the six prices within %.2e of max|U|" % (m1, m2, sR, worst))
                return adm, ref
            print("launchers %dx%d: at s-ratio %.0e the references differ by %.2e of max|U| on a price" % (m1, m2, sR, worst))
        sR /= 10
        assert sR >= 1e2, "no s-ratio at which the references agree"


LAUNCHERS = [("lds_50x25", 50, 25, {"small_seq": 1}, ["hadi_small_seq_kernel<1>"], ["hadi_small_"]),
             ("strips_300x80", 300, 80, _st(strip=1), ["hadi_pass_a_strip<8,EU>"], ["hadi_pass_a_strip<8,AM"])]


@pytest.mark.parametrize("sR", [1e4, 1e6], ids=["s1e4", "s1e6"])
@pytest.mark.parametrize("variant", [H.EU, H.AM_DIV], ids=["EU", "AM_DIV"])
@pytest.mark.parametrize("name,m1,m2,tuning,want_eu,want_am", LAUNCHERS, ids=[c[0] for c in LAUNCHERS])
def test_launchers(solver, name, m1, m2, tuning, want_eu, want_am, variant, sR):
    """compute_base_prices* and compute_jacobian* with S_0 beside a raw s-node and every V_0_i beside a raw v-node: the device
    rebuilds each instance's v-grid for V_0_i and for V_0_i + eps.  A price is one node of the field and is judged by the field
    rule at that node; J through its reconstructed prices base + eps J_g, each by the same rule (the yardstick is the base
    sweep's: a bump of 1e-6 in a parameter does not move the conditioning of the grid).  |J - J_oracle| is printed only: a
    difference quotient over eps = 1e-6 carries (price round-off) / eps."""
    N = 10 if variant == H.AM_DIV else 4
    c = I.cfg(N, r_f=R_F, variant=OV[variant])
    insts, ref = _admitted_launcher_instances(c, m1, m2, sR)
    strikes, grids, U0 = gridviews(insts)
    n0, total = len(insts), (m1 + 1) * (m2 + 1)
    g = [I.grids(i) for i in insts]
    s0, v0s = g[0][4], [x[5] for x in g]
    assert all(x[4] == s0 for x in g)
    args = (Cm.T, Cm.R_D, R_F, *c.model, m1, m2, total, N, Cm.THETA, Cm.T / N, n0, grids)
    ws = H.DOWorkspace(n0, total)
    ws.U[...] = U0
    per, div = {"V_0_i": v0s}, H.Dividends(*Cm.DIVS)
    with _tuned(solver, tuning):
        if variant == H.EU:
            prices = solver.compute_base_prices(s0, -1.0, *args, ws, per_instance=per)
            J, base = solver.compute_jacobian(s0, -1.0, *args, U0, per_instance=per)
        else:
            prices = solver.compute_base_prices_american_dividends(s0, -1.0, *args, U0, ws, div, per_instance=per)
            J, base = solver.compute_jacobian_american_dividends(s0, -1.0, *args, U0, div, per_instance=per)
        d = solver.describe_last_sweep()
    _has(d, want_eu if variant == H.EU else want_am)
    ok, worst_J, vname = True, 0.0, "EU" if variant == H.EU else "AM_DIV"
    for k, inst in enumerate(insts):
        (po, bo, bumped_o, Jo, scale), (bx, bumped_x, scale_x) = ref[k]
        worst_J = max(worst_J, float(np.abs(J[k] - Jo).max()))
        todo = [("price", prices[k], po, bx), ("base", base[k], bo, bx)]
        todo += [(BUMPS[q], base[k] + EPS * J[k, q], bumped_o[q], bumped_x[q]) for q in range(5)]
        for what, x, x_o, x_x in todo:
            v = I.judge_value(x, x_o, scale, lambda x_x=x_x: (x_x, scale_x), lambda inst=inst: I.yard(c, inst)[0])
            if v["stage"] == "adjudicated" or not v["ok"]:
                print("  %s %s #%d %s, %s: %s" % (name, vname, k, I.describe(inst), what,
                                                  {a: (b if isinstance(b, (bool, str)) or b is None else float("%.3g" % b)) for a, b in v.items()}))
            ok = ok and v["ok"]
    print("%s %s s-ratio %.0e: |J - J_oracle| %.3e (printed only: price round-off / eps)" % (name, vname, insts[0].sR, worst_J))
    assert ok


# ---- f. the post-processing kernels on an ill-conditioned row -------------------------------------------------------------
def _post_batch(m1, m2, t, side, sR, vR):
    """Two instances for the calls that take ONE (S_0, V_0): both on the v-grid whose V_0 sits h / vR beside the raw node below
    0.04; instance 0 with S_0 placed so that the finished tiny s-interval is [t, t + 1], instance 1 (another strike) with the same
    S_0 inserted wherever it falls on its own grid."""
    K0, K1 = Cm.well_conditioned_strikes(m1, 2)
    raw = I.raw_s(m1, K0)
    si = t if side == "lower" else t - 1
    vs0, ds0, s0 = I.s_grid(m1, K0, si, I.fit_ratio(raw[si + 1] - raw[si], sR), side)
    g1 = O.grid(m1, 8 * K1, s0, K1, K1 / 5, 4, 5.0, 0.04, 0.01)
    raw_v = I.raw_v(m2)
    j = next(x for name, kind, x in I.v_positions(m2) if name.startswith("holds V_0"))
    vv, dv, v0 = I.v_grid(m2, j, I.fit_ratio(raw_v[j + 1] - raw_v[j], vR), "lower")
    g = object.__new__(H.GridViewsBatch)
    g.m1, g.m2, g.n = m1, m2, 2
    g.Vec_s, g.Delta_s = np.ascontiguousarray(np.stack([vs0, g1[0]])), np.ascontiguousarray(np.stack([ds0, g1[2]]))
    g.Vec_v, g.Delta_v = np.ascontiguousarray(np.stack([vv, vv])), np.ascontiguousarray(np.stack([dv, dv]))
    assert len(I.find_all(g1[0], s0)) == 1 and (np.diff(g1[0]) > 0).all()
    return [float(K0), float(K1)], g, g.call_payoff([K0, K1]), s0, v0


def _s_target(m1, where):
    K0 = Cm.well_conditioned_strikes(m1, 2)[0]
    if where == "tile_edge":  # HADI_GK_TILE = 512 nodes per block on rows in natural order: nodes 511 | 512
        assert I.E.pick_shape(m1)[0] == 1 and m1 > 1024
        return 511
    return next(x for name, kind, x in I.s_positions(m1, K0) if name == "holds 100")


GREEKS = [("50x25", 50, 25, {"small_seq": 0}, ["hadi_small_kernel<1,"], "beside_100", "lower"),
          ("300x80", 300, 80, _st(strip=1), ["hadi_pass_a_strip<8,EU>"], "beside_100", "upper"),
          ("1100x30", 1100, 30, _st(), ["hadi_pass_a_seq<EU>"], "beside_100", "lower"),
          ("1100x30_tile_edge", 1100, 30, _st(), ["hadi_pass_a_seq<EU>"], "tile_edge", "lower")]


@pytest.mark.parametrize("name,m1,m2,tuning,want,where,side", GREEKS, ids=[c[0] for c in GREEKS])
def test_greeks_kernel_alone_on_an_ill_conditioned_row(solver, name, m1, m2, tuning, want, where, side):
    """compute_greeks with the ladder, then DO_timestepping of the same batch on the same handle under the same tuning (same
    description, same bits); greeks_ref on THAT field at the rounding-level bound, price and lambda columns bit for bit.  The
    stencil weights on the tiny intervals are 1e4 .. 1e6 times the usual ones: the bound carries them (stencil_norms)."""
    N = 3
    strikes, grids, U0, s0, v0 = _post_batch(m1, m2, _s_target(m1, where), side, 1e6, 1e4)
    head = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids)
    with _tuned(solver, tuning):
        greeks, lad = solver.compute_greeks(*head, U0.copy(), s0, v0, ladder=True)
        d1 = solver.describe_last_sweep()
        U = U0.copy()
        solver.DO_timestepping(*head, U)
        d2 = solver.describe_last_sweep()
    _has(d1, want)
    assert d1 == d2, (d1, d2)
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
    for k in range(2):
        g = (grids.Vec_s[k], grids.Vec_v[k], grids.Delta_s[k], grids.Delta_v[k])
        b = G.boundary_vector(p, *g, U0[k])[0]
        j0, i0 = G.find_node(g[1], v0), G.find_node(g[0], s0)
        assert i0 >= 0 and j0 >= 0
        ref = G.ladder(p, *g, U[k], None, j0, b)
        bound = G.rounding_bound(p, g[0], g[1], j0, np.abs(U[k]).max())
        r, at = G.worst_ratio(lad[k], ref, bound)
        print("%s instance %d (s-intervals %.1ex apart): worst |diff| / bound %.3e at node %d column %s" % (
            name, k, Cm.interval_ratios(g[2])[0], r, at[0], G.NAMES[at[1]]))
        assert r <= 1.0, "instance %d node %d column %s: got %.17g ref %.17g bound %.3e" % (
            k, at[0], G.NAMES[at[1]], lad[k][at], ref[at], bound[at])
        assert np.array_equal(lad[k, :, G.PRICE], ref[:, G.PRICE]) and np.array_equal(lad[k, :, G.LAMBDA], ref[:, G.LAMBDA])
        assert np.array_equal(greeks[k], lad[k, i0])


def _spots_around(vs, a):
    """Inside the tiny interval [a, a + 1], in the two intervals beside it, on both of its end nodes, and in the first and the
    last interval of the grid, whose clamped four-node stencils span the tiny interval when it lies within them."""
    m1 = len(vs) - 1
    mid = lambda i, f: float(vs[i] + f * (vs[i + 1] - vs[i]))
    return [mid(a, 0.4), mid(max(a - 1, 0), 0.7), mid(min(a + 1, m1 - 1), 0.3), float(vs[a]), float(vs[a + 1]), mid(0, 0.45), mid(m1 - 1, 0.55)]


SAMPLES = [("50x25", 50, 25, {"small_seq": 0}, ["hadi_small_kernel<"]), ("300x80", 300, 80, _st(strip=1), ["hadi_pass_a_strip<8,EU>"]),
           ("600x40", 600, 40, _st(), ["hadi_pass_a<8,2,"])]


@pytest.mark.parametrize("turn", [0, 1])
@pytest.mark.parametrize("name,m1,m2,tuning,want", SAMPLES, ids=[c[0] for c in SAMPLES])
def test_sample_kernel_alone_on_an_ill_conditioned_row(solver, name, m1, m2, tuning, want, turn):
    """sample_ladder at the last step, then DO_timestepping of the same batch under the same tuning (the same sweep kernels in
    the description); samples_ref on THAT field.  Bound: the file's own form sum|w| |scale| max|U| with the rounding-level factor
    of greeks_ref.rounding_bound (1e-13) in place of 1e-10; a spot on a node returns the node's value bit for bit."""
    N = 3
    insts = I.batch(m1, m2, len(I.s_positions(m1, 100.0)), "s", turn)
    insts = tuple(i._replace(v0=insts[0].v0) for i in insts)  # (one scalar V_0 for the batch)
    strikes, grids, U0 = gridviews(insts)
    v0 = insts[0].v0
    tiny = [int(np.argmin(grids.Delta_s[k])) for k in range(len(insts))]
    spots = np.ascontiguousarray(np.array([_spots_around(grids.Vec_s[k], tiny[k]) for k in range(len(insts))]))
    # (r_f = 0: with r_f != 0 the call boundary data carry exp(-r_f dt (N - 1)) and the library refuses a ladder)
    head = (m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids)
    with _tuned(solver, tuning):
        out = solver.sample_ladder(*head, U0.copy(), spots, v0, [N])
        d1 = solver.describe_last_sweep()
        U = U0.copy()
        solver.DO_timestepping(*head, U)
        d2 = solver.describe_last_sweep()
    _has(d1, want + ["sampled ladder: 1 snapshots x 7 samples"])
    _has(d2, want)
    kernels = lambda d: set(re.findall(r"hadi_\w+<[^>]*>", d)) - {x for x in re.findall(r"hadi_\w+<[^>]*>", d) if x.startswith("hadi_sample")}
    assert kernels(d1) == kernels(d2), (d1, d2)
    ref, amp, flags = SR.sample_batch(U, grids.Vec_s, grids.Vec_v, v0, spots)
    assert (flags == 0).all()
    bound = G.ROUNDING_EPS * amp * np.abs(U).max(axis=1, keepdims=True)
    diff = np.abs(out[:, 0, :] - ref)
    print("%s turn %d: sum|w| up to %.2e, worst |diff| / bound %.3e" % (name, turn, amp.max(), (diff / bound).max()))
    assert (diff <= bound).all(), (np.argwhere(diff > bound)[:4], (diff / bound).max())
    assert np.array_equal(out[:, 0, 3:5], ref[:, 3:5])  # the two end nodes of the tiny interval


def shapes_used():
    """Every (m1, m2, sweep) of sections a - d, for tests/test_oracle_ill_grids.py: (m1, m2, N, theta, r_f, variant, scheme, put)."""
    out = set()
    for name, m1, m2, n, tuning, want, absent, kw in FAMILIES:
        out.add((m1, m2, 3, Cm.THETA, R_F, OV[kw.get("variant", H.EU)], 0, False))
    for name, m1, m2, N, tuning, want, absent, kw in VARIANT_ROWS:
        out.add((m1, m2, N, Cm.THETA, R_F, OV[kw.get("variant", H.EU)], 0, kw.get("put", False)))
    for m1, m2 in ((128, 64), (300, 80), (50, 25), (100, 20)):
        out.add((m1, m2, 3, 0.5, 0.007, O.EU, 1, False))
    for name, m1, m2, N, n, variant, kernel in TEAM:
        out.add((m1, m2, N, Cm.THETA, R_F, OV[variant], 0, False))
    out.add((300, 80, 3, Cm.THETA, R_F, O.EU, 0, False))
    return out
