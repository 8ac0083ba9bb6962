"""hadi_small_jump_kernel<B, W> -- the whole-loop kernel of a sampled Bates ladder -- on the device over its domain: the table of
tests/bates_domain_cases.py (tests/test_emu_bates_samples.py and tests/test_emu_small_jump_stage.py walk it under the emulator).
tests/test_gpu_bates_samples.py runs 50x25 and 100x12 with three instances, ten unscaled samples and "jump_small" pinned; this file
runs
  a. every shape of the table at W = 4 and 8 (all four instantiations by name), the lambda = 0 instance against the plain block
     kernel of the same <B, W> bit for bit;
  b. puts with dividends that pay inside the sweep on the two extreme shapes;
  c. the automatic rule ("jump_small" = -1) at n = cu - 1, cu, 2 cu and 2 cu + 1 instances, cu the device's own count: more than one
     block per CU, every instance against its first twin bit for bit; once more with delta_t_i;
  d. the Jacobian with eight and five columns on the automatic route: the per-instance matrix index over nine groups and three
     matrix sets at 9 n0 >= cu and 9 n0 > 2 cu;
  e. 1 .. 1024 samples per instance (hadi_sample_lds with strides of 256 and 512 threads);
  f. a second jump law on the same handle at the same shape, per-instance and shared-grid.
Bounds: bates_domain_cases' (the project's own).  The reference runs on the distinct instances only.  The sub-step alone cannot be
isolated here -- a device call always includes the Douglas step --; tests/test_emu_small_jump_stage.py does that."""
import contextlib

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import bates_domain_cases as BD
import common as Cm
import dividend_schedules as D
import samples_ref as SR

pytestmark = pytest.mark.gpu

DEFAULTS = {"jump_small": -1, "small_waves": 0, "small_seq": -1}
LOOP_WORDS = "; Bates: jump sub-step on the fp64 matrix core inside the time loop"
JUMP_WORDS = "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step"
SEL_WORDS = "; Bates: hadi_jump_sel_kernel (fp64 matrix core, three matrix sets picked by group) behind the last column pass of every step"


@contextlib.contextmanager
def tuned(sv, **kw):
    """The handle is shared by the session: every key goes back to its default."""
    try:
        for k, v in kw.items():
            sv.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            sv.set_tuning(k, DEFAULTS[k])


def device_grids(m1, m2, strikes, V_0):
    g = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, V_0, strikes)
    return g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, g.call_payoff(strikes)


def distinct(m1, m2, d, **kw):
    return BD.distinct(m1, m2, d, make_grids=device_grids, **kw)


def views(b, m1, m2):
    g = object.__new__(H.GridViewsBatch)
    g.m1, g.m2, g.n = m1, m2, b["vs"].shape[0]
    g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v = b["vs"], b["vv"], b["ds"], b["dv"]
    return g


def _kw(b, put, div, dts):
    kw = dict(variant=H.DIV if div else H.EU, dividends=H.Dividends(*Cm.DIVS) if div else None, scales=b["scales"],
              per_instance={"delta_t_i": list(dts)} if dts is not None else None)
    if put:
        kw.update(option_type=H.PUT, strikes=list(b["strikes"]))
    return kw


def ladder(sv, dist, b, N, snaps, law=None, div=False, dts=None, shared=False, spots=None):
    law = (b["lam"], b["mu"], b["sig"]) if law is None else law
    kw = _kw(b, dist.put, div, dts)
    if spots is not None:
        kw["scales"] = None
    out = sv.bates_sample_ladder(dist.m1, dist.m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *BD.MODEL, views(b, dist.m1, dist.m2), b["U0"].copy(),
                                 b["spots"] if spots is None else spots, dist.V_0, list(snaps), *law, shared_grid=shared, **kw)
    return out, sv.describe_last_sweep()


def plain_ladder(sv, dist, b, N, snaps, div=False):
    out = sv.sample_ladder(dist.m1, dist.m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *BD.MODEL, views(b, dist.m1, dist.m2), b["U0"].copy(),
                           b["spots"], dist.V_0, list(snaps), **_kw(b, dist.put, div, None))
    return out, sv.describe_last_sweep()


def loop_name(m1, W):
    return "hadi_small_jump_kernel<%d,%d>" % (BD.geometry(m1, 8)[0], W)


def is_loop(d, m1, W, n_snap, n_samp):
    return d.startswith(loop_name(m1, W) + ": whole time loop in one launch") and \
        d.endswith("sampled ladder: %d snapshots x %d samples evaluated inside the time loop%s" % (n_snap, n_samp, LOOP_WORDS))


def is_streaming(d, n_snap, n_samp, sel=False):
    return "row pass" in d and "hadi_small_" not in d and d.endswith(SEL_WORDS if sel else JUMP_WORDS) and \
        ("sampled ladder: %d snapshots x %d samples, hadi_sample_kernel after each snapshot step" % (n_snap, n_samp)) in d


_LARGEST = {}


def largest_m2(sv):
    """The first m2 at 128 whose description no longer starts with hadi_small_jump_kernel<2, -- found with one-step calls of one
    instance, "jump_small" pinned to 1; m2 + 1 streams (asserted by its words)."""
    if "m2" not in _LARGEST:
        seen = {}

        def takes_the_loop(m1, m2):
            g = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.v0_for(m2), [100.0])
            sv.bates_sample_ladder(m1, m2, 1, Cm.T / 4, Cm.THETA, Cm.R_D, Cm.R_F, *BD.MODEL, g, g.call_payoff([100.0]), [Cm.S_0],
                                   Cm.v0_for(m2), [1], 0.5, -0.1, 0.15)
            seen[m2] = sv.describe_last_sweep()
            return seen[m2].startswith("hadi_small_jump_kernel<2,")

        with tuned(sv, jump_small=1):
            m2 = BD.largest_m2(takes_the_loop)
        assert is_streaming(seen[m2 + 1], 1, 1), seen[m2 + 1]
        _LARGEST["m2"] = m2
    return _LARGEST["m2"]


def row_of(sv, m1, m2):
    if m2 is not None:
        return next(r for r in BD.FIXED if (r.m1, r.m2) == (m1, m2))
    return BD.shapes(largest_m2(sv))[-1]


ROWS = [(r.m1, r.m2) for r in BD.FIXED] + [(BD.LARGEST_M1, None)]
ROW_IDS = ["%dx%s" % (a, b if b is not None else "largest") for a, b in ROWS]


# ---- a. every shape x W -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", BD.WIDTHS)
@pytest.mark.parametrize("m1,m2", ROWS, ids=ROW_IDS)
def test_every_shape_at_both_widths(solver, m1, m2, W):
    row = row_of(solver, m1, m2)
    m2, N, snaps = row.m2, 3, [1, 3]
    print(BD.what(row))
    dist = distinct(m1, m2, 3)
    b, _ = BD.replicated(dist, 3)
    assert b["lam"][2] == 0.0 and b["lam"][0] != 0.0 and b["lam"][1] != 0.0
    n_samp = b["spots"].shape[1]
    B = BD.geometry(m1, m2)[0]
    with tuned(solver, jump_small=1, small_waves=W):
        out, d = ladder(solver, dist, b, N, snaps)
    assert is_loop(d, m1, W, 2, n_samp), d
    name = "%dx%d <%d,%d>" % (m1, m2, B, W)
    BD.within_bound(name, out, dist.ref(N, snaps))
    BD.tight(name, out, b["vs"], b["spots"], b["scales"], dist.kinds)
    with tuned(solver, small_seq=0, small_waves=W):
        plain, d0 = plain_ladder(solver, dist, b, N, snaps)
    assert d0.startswith("hadi_small_kernel<%d,%d,EU>" % (B, W)) and "Bates" not in d0, d0
    assert np.array_equal(out[2], plain[2]), "the instance with lambda = 0 is not its plain run"
    for k in (0, 1):
        assert np.abs(out[k] - plain[k]).max() > 1e-6, k


# ---- b. puts with dividends ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", BD.WIDTHS)
@pytest.mark.parametrize("m1,m2", [(16, 11), (BD.LARGEST_M1, None)], ids=["16x11", "128xlargest"])
def test_puts_with_dividends_that_pay_inside_the_sweep(solver, m1, m2, W):
    m2, N, snaps = row_of(solver, m1, m2).m2, 10, [3, 10]
    paid = sorted(D.paying_steps(N, Cm.T / N, Cm.DIVS[0]))  # (the dating mirror: on 4 or 6 steps the canonical schedule pays once or never)
    assert paid == [2, 4, 8] and paid[0] <= snaps[0] < paid[-1] <= N, paid  # (a dividend in front of each snapshot)
    dist = distinct(m1, m2, 3, put=True, first=1)
    b, _ = BD.replicated(dist, 3)
    with tuned(solver, jump_small=1, small_waves=W):
        out, d = ladder(solver, dist, b, N, snaps, div=True)
    assert is_loop(d, m1, W, 2, b["spots"].shape[1]), d
    name = "DIV puts %dx%d W = %d" % (m1, m2, W)
    BD.within_bound(name, out, dist.ref(N, snaps, div=True))
    BD.tight(name, out, b["vs"], b["spots"], b["scales"], dist.kinds)


# ---- c. the automatic rule ---------------------------------------------------------------------------------------------------------
def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def twins_and_bound(name, out, twin, dist, ref, b):
    d = dist.d
    assert np.array_equal(out, out[twin]), "instances %s differ from their first twins" % (np.nonzero((out != out[twin]).any(axis=(1, 2)))[0][:8],)
    BD.within_bound(name, out[:d], ref)
    BD.tight(name, out[:d], b["vs"][:d], b["spots"][:d], b["scales"][:d], dist.kinds)


@pytest.mark.parametrize("which", ["cu-1", "cu", "2cu", "2cu+1"])
@pytest.mark.parametrize("m1,m2", [(50, 25), (100, 12)], ids=["50x25", "100x12"])
def test_the_automatic_rule(solver, m1, m2, which):
    cu = cu_count()
    n = {"cu-1": cu - 1, "cu": cu, "2cu": 2 * cu, "2cu+1": 2 * cu + 1}[which]
    N, snaps = 4, [2, 4]
    dist = distinct(m1, m2, 5)
    b, twin = BD.replicated(dist, n)
    assert solver.get_tuning("jump_small") == -1 and solver.get_tuning("small_waves") == 0
    out, d = ladder(solver, dist, b, N, snaps)
    n_samp = b["spots"].shape[1]
    if which == "cu-1":
        assert is_streaming(d, 2, n_samp), d
    else:
        assert is_loop(d, m1, 4 if which == "2cu+1" else 8, 2, n_samp), d
    twins_and_bound("automatic %dx%d n = %s = %d" % (m1, m2, which, n), out, twin, dist, dist.ref(N, snaps), b)


def test_the_automatic_rule_with_delta_t_i(solver):
    """Fifteen distinct instances: five laws and strikes against three maturities, more than two blocks per CU."""
    m1, m2, N, snaps = 50, 25, 4, [2, 4]
    n = 2 * cu_count() + 1
    dist = distinct(m1, m2, 15)
    dts = [(Cm.T / N, 0.5 / N, 0.8 / N)[k % 3] for k in range(15)]
    b, twin = BD.replicated(dist, n)
    out, d = ladder(solver, dist, b, N, snaps, dts=[dts[k] for k in twin])
    assert is_loop(d, m1, 4, 2, b["spots"].shape[1]), d
    twins_and_bound("automatic, delta_t_i, n = %d" % n, out, twin, dist, dist.ref(N, snaps, dts=dts), b)


# ---- d. the Jacobian on the automatic route -------------------------------------------------------------------------------------------
def jacobian(sv, dist, b, N, snaps, cols8):
    n = b["vs"].shape[0]
    size = (dist.m1 + 1) * (dist.m2 + 1)
    J, base = sv.compute_jacobian_bates_samples(b["spots"], dist.V_0, Cm.R_D, Cm.R_F, *BD.MODEL, dist.m1, dist.m2, size, N, Cm.THETA, Cm.T / N,
                                                n, views(b, dist.m1, dist.m2), b["U0"].copy(), list(snaps), b["lam"], b["mu"], b["sig"],
                                                jump_columns=cols8, scales=b["scales"], eps=BD.EPS)
    return J, base, sv.describe_last_sweep()


@pytest.mark.parametrize("which", ["9n0>=cu", "9n0>2cu"])
@pytest.mark.parametrize("m1,m2", BD.JAC_SHAPES, ids=[BD.row_id(s) for s in BD.JAC_SHAPES])
def test_jacobian_on_the_automatic_route(solver, m1, m2, which):
    cu = cu_count()
    n0 = -(-cu // 9) if which == "9n0>=cu" else (2 * cu) // 9 + 1
    assert (cu <= 9 * n0 <= 2 * cu) if which == "9n0>=cu" else 9 * n0 > 2 * cu
    W8 = 8 if which == "9n0>=cu" else 4
    N, snaps = 4, [2, 4]
    assert m1 <= 100  # (the Jacobian's bound is the project's for rows of at most 100 nodes)
    dist = distinct(m1, m2, 3)
    b, twin = BD.replicated(dist, n0)
    n_samp = b["spots"].shape[1]
    assert solver.get_tuning("jump_small") == -1 and solver.get_tuning("small_waves") == 0
    J8, b8, d8 = jacobian(solver, dist, b, N, snaps, True)
    J5, b5, d5 = jacobian(solver, dist, b, N, snaps, False)
    assert J8.shape == (n0, 2, n_samp, 8) and J5.shape == (n0, 2, n_samp, 5) and b8.shape == b5.shape == (n0, 2, n_samp)
    assert is_loop(d8, m1, W8, 2, n_samp), d8
    # the five-column call has 6 n0 instances: the rule is asserted for it as well
    if 6 * n0 < cu:
        assert is_streaming(d5, 2, n_samp), d5
    else:
        assert is_loop(d5, m1, 8 if 6 * n0 <= 2 * cu else 4, 2, n_samp), d5
    name = "%dx%d n0 = %d" % (m1, m2, n0)
    Jo, bo, amp = dist.ref_jacobian(N, snaps, 8)
    BD.jacobian_within_bounds(name + ", 8 columns " + d8[:27], J8[:3], b8[:3], Jo, bo, amp)
    BD.jacobian_within_bounds(name + ", 5 columns " + d5[:27], J5[:3], b5[:3], Jo[..., :5], bo, amp)
    for X in (J8, b8, J5, b5):
        assert np.array_equal(X, X[twin])
    # bit for bit on ONE kernel: where the rule gave the five-column call another kernel, it is pinned to the eight-column call's
    if d5.split(":")[0] != d8.split(":")[0]:
        with tuned(solver, jump_small=1, small_waves=W8):
            J5, b5, d5 = jacobian(solver, dist, b, N, snaps, False)
        assert is_loop(d5, m1, W8, 2, n_samp), d5
    assert np.array_equal(b8, b5) and np.array_equal(J8[..., :5], J5)
    # lambda_k = 0: the groups 7 and 8 are skipped as group 0 is -- exact zeros; the lambda column is not zero
    zero = np.nonzero(b["lam"] == 0.0)[0]
    assert zero.size and not J8[zero][..., 6:].any() and (np.abs(J8[zero[0], -1, :, 5]) > 0).any()
    assert (np.abs(J8[0, -1, :, 5:]).max(axis=0) > 1e-4).all()


# ---- e. sample counts -----------------------------------------------------------------------------------------------------------------
COUNTS = (1, 255, 256, 257, 511, 513, 1024)
assert set(COUNTS) <= set(BD.SC.COUNTS)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("m1,m2,W", [(50, 25, 4), (100, 12, 8)], ids=["<1,4>", "<2,8>"])
def test_sample_counts(solver, m1, m2, W, count):
    """hadi_sample_lds with 256 and 512 threads: below, at and above one stride, two strides, the documented maximum."""
    N, snaps = 2, [1, 2]
    dist = distinct(m1, m2, 2, first=3, budget=1024, count=count)
    b = dist.fields()
    ten = np.ascontiguousarray(np.stack([SR.kernel_test_spots(b["vs"][k], Cm.S_0) for k in range(2)]))
    with tuned(solver, jump_small=1, small_waves=W):
        out, d = ladder(solver, dist, b, N, snaps)
        out10, d10 = ladder(solver, dist, b, N, snaps, spots=ten)
    assert out.shape == (2, 2, count) and is_loop(d, m1, W, 2, count) and is_loop(d10, m1, W, 2, 10), (d, d10)
    name = "%d samples %s" % (count, loop_name(m1, W))
    BD.within_bound(name, out, dist.ref(N, snaps))
    if count > 1:
        BD.tight(name, out, b["vs"], b["spots"], b["scales"], dist.kinds)
    assert ten[0, 0] == Cm.S_0 == b["spots"][0, 0] and np.array_equal(out[:, :, 0], out10[:, :, 0])


# ---- f. law changes on one handle at one shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1], ids=["streaming", "whole-loop"])
def test_a_second_law_on_the_same_handle_and_shape(solver, route):
    """A matrix (or a weight, or a matrix index) left over from the previous call would show: A, B, A again."""
    m1, m2, N, snaps = 50, 25, 4, [2, 4]
    dist = distinct(m1, m2, 3)
    b = dist.fields()
    A, Bl = BD.laws(3), BD.laws(3, first=2)
    n_samp = b["spots"].shape[1]
    named = (lambda d: is_loop(d, m1, 8, 2, n_samp)) if route else (lambda d: is_streaming(d, 2, n_samp))
    with tuned(solver, jump_small=route):
        a1, dA = ladder(solver, dist, b, N, snaps, law=A)
        b1, dB = ladder(solver, dist, b, N, snaps, law=Bl)
        a2, _ = ladder(solver, dist, b, N, snaps, law=A)
        assert named(dA) and named(dB), (dA, dB)
        assert np.array_equal(a1, a2) and np.abs(b1 - a1).max() > 1e-6
        BD.within_bound("law A, route %d" % route, a1, dist.ref(N, snaps, law=A))
        BD.within_bound("law B, route %d" % route, b1, dist.ref(N, snaps, law=Bl))
        # one grid for the batch, one (mu_J, sigma_J): the shared matrix
        same = distinct(m1, m2, 3, same=True)
        s = same.fields()
        SA, SB = (np.array([0.5, 0.0, 2.0]), -0.10, 0.15), (np.array([1.0, 0.3, 0.0]), 0.05, 0.20)
        sa1, dS = ladder(solver, same, s, N, snaps, law=SA, shared=True)
        sb1, _ = ladder(solver, same, s, N, snaps, law=SB, shared=True)
        sa2, _ = ladder(solver, same, s, N, snaps, law=SA, shared=True)
        assert named(dS), dS
        assert np.array_equal(sa1, sa2) and np.abs(sb1 - sa1).max() > 1e-6
        BD.within_bound("shared law A, route %d" % route, sa1, same.ref(N, snaps, law=SA))
        BD.within_bound("shared law B, route %d" % route, sb1, same.ref(N, snaps, law=SB))
