"""Ill-conditioned grids on purpose, and the rule that judges a solver on them.  Plain data and numpy, shared
by tests/test_oracle_ill_grids.py (the conditions), tests/test_emu_ill_grids.py (wave emulator) and tests/test_gpu_ill_grids.py.

The raw sinh grid of Grid(m1, 8K, x, K, K/5, ...) does not depend on the inserted value x (an x at or above the last raw node is
dropped again, which leaves the raw grid), so inserting x = s_i + h_i / R makes an interval h_i / R beside a neighbour of about
h_i; rebuild_variance(m2, v_j + h_j / R) does the same on the v-axis.  The tiny interval is PLACED: on the s-axis relative to the
lanes and wavefronts of the row pass (wave g, lane l own the nodes 1 + 64 B g + B l + r, r < B: hadi_slot_to_i, as
tests/event_cases.py takes it), on the v-axis relative to the column chunks (HADI_LC = 33 rows), the row strips and the last two
rows of A2.

The rule, per instance (judge): finite; the sanity cap against the fp64 reference (field 1e-4 max|U_o|, lambda_bar 1e-3
max(1, |lambda_o|)); inside the well-conditioned band (1e-10 / 1e-8) nothing further; otherwise the binary128 oracle decides:
e_h = |U - U_x| / max|U_x| < max(30 yard, 1e-11) (lambda_bar: floor 1e-9) -- the numbers of tools/fuzz_parity.py::judge.  `yard` is
the largest of the fp64 oracle's own distance from binary128 on the instance's grid and on its two siblings (same R, same side,
the tiny interval one raw interval down and one up): both distances are single realisations of cond * eps whose ratio moves
between 0.2 and 10 with the position of the interval, so the yardstick is taken over the neighbourhood and fixed before any
solver under test runs.  It is computed lazily, for instances outside the band only."""
import collections
import functools

import numpy as np

from oracle import oracle as O

import common as Cm
import event_cases as E

MIN_INTERVAL = 1e-8   # 100x the node-pick tolerance (1e-10) of find_s_index / find_v_index
RATIOS = (1e4, 1e6)
# axis "both": (R_s, R_v).  The reference's distance from binary128 grows like the product of the two ratios; with 1e6 on both axes
# the fp64 oracle itself was measured up to 8e-6 from binary128 on 50x25 (and 8e-5 with the v-interval at the last row), which
# leaves less than the 31x the sanity cap of 1e-4 needs -- the reference alone could trip it.  So at most one axis carries 1e6.
BOTH_RATIOS = ((1e4, 1e4), (1e6, 1e4), (1e4, 1e6))
SIDES = ("lower", "upper")
LC = 33               # HADI_LC: rows per chunk of the column pass
CAP_U, CAP_L = 1e-4, 1e-3
BAND_U, BAND_L = 1e-10, 1e-8
FLOOR_U, FLOOR_L = 1e-11, 1e-9
FACTOR = 30.0

# One instance: strike K, the tiny s-interval (raw interval si, ratio sR, side s_side; si None: S_0 = 100 inserted, well-conditioned),
# the tiny v-interval likewise (vj None: the well-conditioned grid of V_0 = v0 at V = 5, d = 0.01), and the position names.
Inst = collections.namedtuple("Inst", "m1 m2 K si sR s_side vj vR v_side v0 sname vname")
# One sweep: what the reference solves on an instance's grids.
Cfg = collections.namedtuple("Cfg", "N theta r_f variant scheme put divs model")


def cfg(N, theta=Cm.THETA, r_f=0.01, variant=O.EU, scheme=0, put=False, divs=None, model=None):
    if divs is None and variant in (O.DIV, O.AM_DIV):
        divs = tuple(tuple(x) for x in Cm.DIVS)
    return Cfg(N, theta, r_f, variant, scheme, put, divs, model or (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA))


def find_all(x, x0):
    """Every node within the pick tolerance of x0."""
    return np.nonzero(np.abs(np.asarray(x) - x0) < 1e-10)[0]


def fit_ratio(h, R):
    """R, or the largest power of ten below it that keeps h / R >= MIN_INTERVAL (printed when it drops)."""
    R0 = R
    while h / R < MIN_INTERVAL and R > 10:
        R /= 10.0
    if R != R0:
        print("interval %.3e: R = %.0e drops to %.0e (every interval >= %.0e)" % (h, R0, R, MIN_INTERVAL))
    return R


def _place(raw, i, R, side):
    h = raw[i + 1] - raw[i]
    return float(raw[i] + h / R) if side == "lower" else float(raw[i + 1] - h / R)


def _check(x, dx, node, R):
    """The conditions of a finished axis: asserted, never filtered."""
    assert (np.diff(x) > 0).all(), "not strictly increasing"
    assert np.array_equal(dx, x[1:] - x[:-1])
    assert dx.min() >= MIN_INTERVAL, dx.min()
    assert Cm.interval_ratios(dx)[0] >= R / 2, (Cm.interval_ratios(dx)[0], R)
    hit = find_all(x, node)
    assert len(hit) == 1 and x[hit[0]] == node, (hit, node)
    return int(hit[0])


def raw_s(m1, K):
    """The raw s-grid: the builder with an inserted value it drops again."""
    return O.grid(m1, 8 * K, 16.0 * K, K, K / 5, 4, 5.0, 0.04, 0.01)[0]


def raw_v(m2, V=5.0, d=0.01):
    return O.rebuild_variance(m2, 2.0 * V, V=V, d=d)[0]


def s_grid(m1, K, i, R, side):
    """(Vec_s, Delta_s, x) from the oracle's own builder with x inserted h_i / R inside the lower or the upper end of raw interval
    i.  The tiny interval is finished interval i (lower) or i + 1 (upper); x is finished node i + 1."""
    raw = raw_s(m1, K)
    assert 0 <= i <= (m1 - 1 if side == "lower" else m1 - 2), (i, side)
    x = _place(raw, i, R, side)
    g = O.grid(m1, 8 * K, x, K, K / 5, 4, 5.0, 0.04, 0.01)
    assert _check(g[0], g[2], x, R) == i + 1
    return g[0], g[2], x


def v_grid(m2, j, R, side, V=5.0, d=0.01):
    """(Vec_v, Delta_v, x) from the oracle's rebuild_variance, x = the V_0 of the grid, h_j / R inside raw interval j."""
    raw = raw_v(m2, V, d)
    assert 0 <= j <= (m2 - 1 if side == "lower" else m2 - 2), (j, side)
    x = _place(raw, j, R, side)
    vv, dv = O.rebuild_variance(m2, x, V=V, d=d)
    assert _check(vv, dv, x, R) == j + 1
    return vv, dv, x


# ---- positions ---------------------------------------------------------------------------------------------------------------
# A position is (name, kind, index).  kind "raw": the named raw interval, the tiny interval at the end `side` says.  kind "at":
# the FINISHED tiny interval is [node index, node index + 1] whichever the side (raw interval index for lower, index - 1 for upper).
def s_positions(m1, K):
    B, G = E.pick_shape(m1)
    raw = raw_s(m1, K)
    c = int(np.searchsorted(raw, K, side="right")) - 1       # raw interval that holds the strike
    c100 = int(np.searchsorted(raw, Cm.S_0, side="right")) - 1
    edge = B * (max(c, c100) // B + 2)                         # the last node of a lane, a lane or two above the strike and 100
    assert 2 <= c <= m1 - 4 and edge + 2 <= m1 - 2, (c, edge, m1)
    pos = [("first interval", "raw", 0), ("between two lanes", "at", edge)]
    if B >= 2:
        pos.append(("inside a lane", "at", edge + 1))
    if G >= 2:
        pos.append(("astride two wavefronts", "at", 64 * B))
    pos += [("holds the strike", "raw", c), ("holds 100", "raw", c100), ("last interval", "at", m1 - 1)]
    for name, kind, t in pos:
        if kind == "at" and name != "last interval":          # ownership of the two nodes around the tiny interval
            la, lb = (t - 1) // B, t // B
            assert (la != lb) == (name != "inside a lane"), (name, t, B)
            assert name != "astride two wavefronts" or (t - 1) // (64 * B) != t // (64 * B)
    return pos


def v_positions(m2, strip_rows=None, V=5.0, d=0.01):
    """strip_rows: height of the row pass's strips where it runs strips (None: no strip-edge position)."""
    raw = raw_v(m2, V, d)
    j0 = int(np.searchsorted(raw, Cm.V_0, side="right")) - 1
    pos = [("first interval", "raw", 0), ("holds V_0 = 0.04", "raw", j0)]
    if m2 >= LC + 1:
        pos.append(("rows 32 | 33", "at", LC - 1))
    if strip_rows is not None and 2 <= strip_rows <= m2 - 3 and strip_rows != LC:
        pos.append(("strip edge", "at", strip_rows - 1))
    pos += [("second last interval", "at", m2 - 2), ("last interval", "at", m2 - 1)]
    return pos


def _raw_index(kind, t, side):
    return t if (kind == "raw" or side == "lower") else t - 1


def _pick(pos, k, turn):
    """Position (k + turn) of the list; the ratio and the side follow the POSITION and the turn, so that turn 0 and turn 1
    together give every position both ratios and both sides."""
    p = (k + turn) % len(pos)
    return pos[p], RATIOS[(p + turn) % 2], SIDES[(p // 2 + turn) % 2]


@functools.lru_cache(maxsize=None)
def batch(m1, m2, n, axis, turn, strip_rows=None):
    """n instances (a tuple of Inst), instance k on position (k + turn) of its axis list; the other axis well-conditioned
    (asserted).  axis "both": a tiny interval on each axis."""
    assert axis in ("s", "v", "both")
    strikes = Cm.well_conditioned_strikes(m1, n)
    cand = Cm.mixed_vgrid_candidates(m2, vary_vd=False)
    out = []
    for k, K in enumerate(strikes):
        si = sR = ss = vj = vR = vs = v0 = None
        sname = vname = "well-conditioned"
        both = BOTH_RATIOS[(k + turn) % 3]
        if axis in ("s", "both"):
            (sname, kind, t), R, ss = _pick(s_positions(m1, K), k, turn)
            R = both[0] if axis == "both" else R
            si = _raw_index(kind, t, ss)
            raw = raw_s(m1, K)
            sR = fit_ratio(raw[si + 1] - raw[si], R)
        if axis in ("v", "both"):
            (vname, kind, t), R, vs = _pick(v_positions(m2, strip_rows), k, turn)
            R = both[1] if axis == "both" else R
            vj = _raw_index(kind, t, vs)
            raw = raw_v(m2)
            vR = fit_ratio(raw[vj + 1] - raw[vj], R)
        else:
            v0 = cand[k % len(cand)][1]
        inst = Inst(m1, m2, float(K), si, sR, ss, vj, vR, vs, v0, sname, vname)
        g = grids(inst)
        if si is None:
            assert Cm.interval_ratios(g[2])[0] <= Cm.COND_MAX
        if vj is None:
            assert Cm.interval_ratios(g[3])[0] <= Cm.COND_MAX
        out.append(inst)
    return tuple(out)


def describe(inst):
    s = "" if inst.si is None else "s: %s (raw %d, R %.0e, %s)" % (inst.sname, inst.si, inst.sR, inst.s_side)
    v = "" if inst.vj is None else "v: %s (raw %d, R %.0e, %s)" % (inst.vname, inst.vj, inst.vR, inst.v_side)
    return "; ".join(x for x in (s, v) if x)


def grids(inst):
    """(Vec_s, Vec_v, Delta_s, Delta_v, s-node, v-node): the inserted nodes (S_0 = 100 / V_0 = v0 on a well-conditioned axis)."""
    if inst.si is None:
        g = O.grid(inst.m1, 8 * inst.K, Cm.S_0, inst.K, inst.K / 5, 4, 5.0, 0.04, 0.01)
        vs, ds, xs = g[0], g[2], Cm.S_0
    else:
        vs, ds, xs = s_grid(inst.m1, inst.K, inst.si, inst.sR, inst.s_side)
    if inst.vj is None:
        vv, dv = O.rebuild_variance(inst.m2, inst.v0)
        xv = inst.v0
    else:
        vv, dv, xv = v_grid(inst.m2, inst.vj, inst.vR, inst.v_side)
    return vs, vv, ds, dv, xs, xv


def payoff(inst, vec_s, put=False):
    row = np.maximum(inst.K - vec_s, 0.0) if put else np.maximum(vec_s - inst.K, 0.0)
    return np.tile(row, inst.m2 + 1)


def arrays(insts, put=False):
    """(strikes, Vec_s, Vec_v, Delta_s, Delta_v, U0) of a batch as the [n][...] arrays the solvers take."""
    G = [grids(i) for i in insts]
    vs, vv, ds, dv = (np.ascontiguousarray(np.stack([g[k] for g in G])) for k in range(4))
    U0 = np.ascontiguousarray(np.stack([payoff(i, g[0], put) for i, g in zip(insts, G)]))
    return np.array([i.K for i in insts]), vs, vv, ds, dv, U0


def params(c, inst):
    return O.make_params(inst.m1, inst.m2, c.N, Cm.T / c.N, c.theta, Cm.R_D, c.r_f, *c.model, c.variant, c.divs, scheme=c.scheme,
                         option_type=O.PUT if c.put else O.CALL, strikes=np.array([inst.K]) if c.put else None)


# ---- the two references, the yardstick and the rule --------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def reference(c, insts):
    """(U_o, lambda_o or None) of a batch: the fp64 oracle on 16 threads, every instance on its own grids."""
    ks, vs, vv, ds, dv, U0 = arrays(insts, c.put)
    p = O.make_params(insts[0].m1, insts[0].m2, c.N, Cm.T / c.N, c.theta, Cm.R_D, c.r_f, *c.model, c.variant, c.divs, scheme=c.scheme,
                      option_type=O.PUT if c.put else O.CALL, strikes=ks if c.put else None)
    Uo, lo, _ = O.solve_batch(p, vs, vv, ds, dv, U0, U0, threads=16, want_lambda=True)
    return Uo, lo


@functools.lru_cache(maxsize=64)
def exact(c, inst):
    """(U_x, lambda_x or None): the binary128 oracle on the instance's grids."""
    vs, vv, ds, dv = grids(inst)[:4]
    U0 = payoff(inst, vs, c.put)
    return O.solve_xp(params(c, inst), vs, vv, ds, dv, U0, U0, strike=inst.K if c.put else None)


def distances(U, lam, Ux, lx):
    """(field, lambda_bar or None) distance from the exact result, in the adjudicator's norms."""
    eU = float(np.abs(U - Ux).max() / np.abs(Ux).max())
    eL = None if lx is None or lam is None else float(np.abs(lam - lx).max() / max(1.0, np.abs(lx).max()))
    return eU, eL


@functools.lru_cache(maxsize=4096)
def oracle_distance(c, inst):
    """The fp64 oracle's own distance from its binary128 twin on the instance's grids: (field, lambda_bar or None)."""
    vs, vv, ds, dv = grids(inst)[:4]
    U0 = payoff(inst, vs, c.put)
    Uo, lo, _ = O.solve(params(c, inst), vs, vv, ds, dv, U0, U0)
    assert np.isfinite(Uo).all()
    return distances(Uo, lo, *exact(c, inst))


def _admissible(c, inst):
    eU, eL = oracle_distance(c, inst)
    return eU <= CAP_U / 31 and (eL is None or eL <= CAP_L / 31)


def _admit_one(c, inst):
    while not _admissible(c, inst):
        s_turn = inst.si is not None and (inst.vj is None or inst.sR >= inst.vR)
        R = inst.sR if s_turn else inst.vR
        assert R > 10, ("no ratio keeps the reference within the cap / 31", describe(inst))
        nxt = inst._replace(sR=R / 10) if s_turn else inst._replace(vR=R / 10)
        print("%s: the fp64 oracle is %.2e%s from binary128: R = %.0e drops to %.0e" % (
            describe(inst), oracle_distance(c, inst)[0], "" if oracle_distance(c, inst)[1] is None else " (lambda_bar %.2e)" % oracle_distance(c, inst)[1],
            R, R / 10))
        inst = nxt
    return inst


def admit(c, insts, threads=16):
    """The batch with the condition the sanity cap needs: on every instance the fp64 oracle itself stands within 1 / 31 of the cap
    from binary128 (field 1e-4 / 31, lambda_bar 1e-3 / 31), so that the reference alone never trips the cap while a solver is
    within 30x of it.  Where it does not -- measured: a 1e6 interval astride the two wavefronts of a 600-interval row, at s near
    500 where the s^2 v / ds^2 coefficients are largest, and American sweeps, whose projection turns round-off into a moved
    exercise boundary -- the ratio of THAT instance drops by powers of ten until it does, and the drop is printed.  Decided by
    the two references alone, before any solver under test runs; like the 1e-8 rule it is a condition on the input."""
    from multiprocessing.pool import ThreadPool
    with ThreadPool(max(1, min(threads, len(insts)))) as pool:
        return tuple(pool.map(lambda i: _admit_one(c, i), insts))


def siblings(inst):
    """The instance with its tiny interval(s) one raw interval down and one up: same R, same side.  A sibling that would leave the
    axis, or whose tiny interval would fall below MIN_INTERVAL, does not exist."""
    out = []
    for step in (-1, 1):
        si = None if inst.si is None else inst.si + step
        vj = None if inst.vj is None else inst.vj + step
        ok = True
        if si is not None:
            raw = raw_s(inst.m1, inst.K)
            ok = ok and 0 <= si <= (inst.m1 - 1 if inst.s_side == "lower" else inst.m1 - 2) and (raw[si + 1] - raw[si]) / inst.sR >= MIN_INTERVAL
        if vj is not None:
            raw = raw_v(inst.m2)
            ok = ok and 0 <= vj <= (inst.m2 - 1 if inst.v_side == "lower" else inst.m2 - 2) and (raw[vj + 1] - raw[vj]) / inst.vR >= MIN_INTERVAL
        if ok:
            out.append(inst._replace(si=si, vj=vj))
    return out


def yard(c, inst):
    """(field, lambda_bar or None): the largest oracle distance over the instance and its siblings."""
    d = [oracle_distance(c, i) for i in [inst] + siblings(inst)]
    return max(x[0] for x in d), (None if d[0][1] is None else max(x[1] for x in d))


def before_adjudication(U, Uo, lam=None, lo=None):
    """Steps 1 - 3 of the rule -> (verdict, decided): finite, the sanity cap, the well-conditioned band."""
    out = dict(ok=False, stage="finite", d=None, dl=None)
    if not (np.isfinite(U).all() and (lam is None or np.isfinite(lam).all())):
        return out, True
    out["d"] = d = float(np.abs(U - Uo).max() / np.abs(Uo).max())
    out["dl"] = dl = None if lam is None else float(np.abs(lam - lo).max() / max(1.0, np.abs(lo).max()))
    out["stage"] = "cap"
    if not (d <= CAP_U and (dl is None or dl <= CAP_L)):
        return out, True
    out["stage"] = "band"
    out["ok"] = bool(d < BAND_U and (dl is None or dl < BAND_L))
    return out, out["ok"]


def judge(U, Uo, exact_fn, yard_fn, lam=None, lo=None):
    """One instance by the rule -> dict(ok, stage, d, dl, and after adjudication e_h, e_o, yard, ratio, l_h, l_o, lyard).
    exact_fn() -> (U_x, lambda_x); yard_fn() -> (yard, lambda yard); neither is called unless the instance is outside the band."""
    out, decided = before_adjudication(U, Uo, lam, lo)
    if decided:
        return out
    out["stage"] = "adjudicated"
    Ux, lx = exact_fn()
    e_h, l_h = distances(U, lam, Ux, lx)
    e_o, l_o = distances(Uo, lo, Ux, lx)
    y, ly = yard_fn()
    out.update(e_h=e_h, e_o=e_o, yard=y, ratio=e_h / max(y, 1e-300), l_h=l_h, l_o=l_o, lyard=ly)
    out["ok"] = bool(e_h < max(FACTOR * y, FLOOR_U) and (l_h is None or l_h < max(FACTOR * ly, FLOOR_L)))
    return out


def judge_batch(name, c, insts, U, lam=None, threads=16):
    """Every instance of a batch by the rule against reference(c, insts); prints the adjudicated numbers and returns
    (all ok, the verdicts).  The binary128 solves of the instances outside the band run side by side on `threads` threads."""
    from multiprocessing.pool import ThreadPool
    Uo, lo = reference(c, insts)
    assert np.isfinite(Uo).all()
    if lam is None or lo is None:
        lam = lo = [None] * len(insts)
    todo = [k for k in range(len(insts)) if not before_adjudication(U[k], Uo[k], lam[k], lo[k])[1]]
    with ThreadPool(max(1, min(threads, len(todo)))) as pool:
        adj = dict(zip(todo, pool.map(lambda k: (exact(c, insts[k]), yard(c, insts[k])), todo)))
    verdicts, worst = [], 0.0
    for k, inst in enumerate(insts):
        v = judge(U[k], Uo[k], lambda: adj[k][0], lambda: adj[k][1], lam[k], lo[k])
        verdicts.append(v)
        if v["stage"] == "adjudicated":
            worst = max(worst, v["ratio"])
            print("  %s #%d %s: e_h %.2e e_o %.2e yard %.2e e_h/yard %.2f%s -> %s" % (
                name, k, describe(inst), v["e_h"], v["e_o"], v["yard"], v["ratio"],
                "" if v["l_h"] is None else "; lambda_bar %.2e / %.2e yard %.2e" % (v["l_h"], v["l_o"], v["lyard"]), "ok" if v["ok"] else "FAIL"))
        elif not v["ok"]:
            print("  %s #%d %s: FAIL at %s, d %s dl %s" % (name, k, describe(inst), v["stage"], v["d"], v["dl"]))
    ds_ = [v["d"] for v in verdicts if v["d"] is not None]
    print("%s: %d instances, %d adjudicated, worst |U - U_o| %.2e, worst e_h / yard %.2f" % (
        name, len(insts), sum(v["stage"] == "adjudicated" for v in verdicts), max(ds_) if ds_ else float("nan"), worst))
    return all(v["ok"] for v in verdicts), verdicts


def judge_value(x, x_o, scale_o, exact_fn, yard_fn):
    """The field rule at ONE node (a price): distances over the scale of the instance's field, max|U_ref| against the reference
    and max|U_x| against binary128.  exact_fn() -> (x_x, max|U_x|); yard_fn() -> the field yardstick of the instance."""
    out = dict(ok=False, stage="finite", d=None)
    if not np.isfinite(x):
        return out
    out["d"] = d = float(abs(x - x_o) / scale_o)
    out["stage"] = "cap"
    if not d <= CAP_U:
        return out
    out["stage"] = "band"
    if d < BAND_U:
        out["ok"] = True
        return out
    out["stage"] = "adjudicated"
    x_x, scale_x = exact_fn()
    y = yard_fn()
    e_h, e_o = float(abs(x - x_x) / scale_x), float(abs(x_o - x_x) / scale_x)
    out.update(e_h=e_h, e_o=e_o, yard=y, ratio=e_h / max(y, 1e-300))
    out["ok"] = bool(e_h < max(FACTOR * y, FLOOR_U))
    return out
