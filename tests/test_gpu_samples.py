"""The sampled ladder on the device (hadi_sample_ladder, hadi_compute_base_prices_samples, hadi_compute_jacobian_samples): one case
per execution path, each with its tuning keys pinned so that the sample call and the ladder call it is compared with run the same
kernels.  Ten spots per instance (samples_ref.kernel_test_spots: S_0, two other nodes, five interior off-node spots, one in the
first and one in the last interval).  Everywhere
  - the S_0 column equals maturity_ladder on the same route BIT FOR BIT, and
  - every sample lies within 1e-10 sum|w| |scale| max|U_ref| of samples_ref applied to the oracle's field at N = snap_steps[q]
    (the project's field bound propagated through the stencil; well-conditioned grids, asserted).
Calls run at the canonical r_f = 0, as the ladder's."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle as O

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

import common as Cm
import samples_ref as R
import scheme_ref as S

pytestmark = pytest.mark.gpu

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH_MCS, TH_HV = 1.0 / 3.0, 0.5 + math.sqrt(3.0) / 6.0
VAR = {"EU": H.EU, "AM": H.AM, "DIV": H.DIV, "AM_DIV": H.AM_DIV}
DEFAULTS = {"small_grid": 1, "small_seq": -1, "small_pairs": -1, "small_sch": -1, "american_p": 1, "streams": 0, "strip": -1,
            "resident_sweep": -1, "team_launch": -1, "graph": 1}
N_STEPS, SNAPS = 6, [2, 5, 6]


@contextlib.contextmanager
def tuned(sv, **kw):
    """The handle is shared by the session: every key goes back to its default."""
    for k, v in kw.items():
        sv.set_tuning(k, v)
    try:
        yield
    finally:
        for k in kw:
            sv.set_tuning(k, DEFAULTS[k])


def _v0(m2):
    """V_0 of a well-conditioned v-grid with m2 intervals (the 30x rule is asserted on the finished batch)."""
    ok = lambda v0: Cm.interval_ratios(O.rebuild_variance(m2, v0)[1])[0] <= Cm.COND_MAX
    return Cm.V_0 if ok(Cm.V_0) else Cm.V_0_ALT


_batches = {}


def _batch(m1, m2, n):
    if (m1, m2, n) not in _batches:
        strikes = Cm.well_conditioned_strikes(m1, n)
        grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, _v0(m2), strikes)
        Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
        spots = np.ascontiguousarray(np.stack([R.kernel_test_spots(grids.Vec_s[k], Cm.S_0) for k in range(n)]))
        _batches[(m1, m2, n)] = (strikes, grids, spots)
    return _batches[(m1, m2, n)]


class Case:
    def __init__(self, m1, m2, n=3, N=N_STEPS, variant="EU", scheme=0, theta=Cm.THETA, put=False, dts=None):
        self.m1, self.m2, self.n, self.N, self.variant, self.scheme, self.theta, self.put = m1, m2, n, N, variant, scheme, theta, put
        self.strikes, self.grids, self.spots = _batch(m1, m2, n)
        self.U0 = Cm.put_payoff(self.grids.Vec_s, self.strikes, m2) if put else self.grids.call_payoff(self.strikes)
        self.div = H.Dividends(*Cm.DIVS) if "DIV" in variant else None
        self.dts = dts
        self.v0 = _v0(m2)
        self._fields = {}

    def kw(self):
        k = dict(variant=VAR[self.variant], dividends=self.div, scheme=self.scheme)
        if "AM" in self.variant:
            k["U_0"] = self.U0
        if self.put:
            k.update(option_type=H.PUT, strikes=self.strikes)
        if self.dts:
            k["per_instance"] = {"delta_t_i": self.dts}
        return k

    def head(self, N=None):
        return (self.m1, self.m2, N or self.N, Cm.T / self.N, self.theta, Cm.R_D, Cm.R_F) + MODEL + (self.grids,)

    def samples(self, sv, snaps, spots=None, scales=None):
        out = sv.sample_ladder(*self.head(), self.U0.copy(), self.spots if spots is None else spots, self.v0, snaps, scales=scales,
                               **self.kw())
        return out, sv.describe_last_sweep()

    def ladder(self, sv, snaps):
        out = sv.maturity_ladder(*self.head(), self.U0.copy(), Cm.S_0, self.v0, snaps, **self.kw())
        return out, sv.describe_last_sweep()

    def fields(self, N):
        """The oracle's fields after N steps: computed once per case and N, left unchanged."""
        if N not in self._fields:
            g, out = self.grids, []
            for k in range(self.n):
                dt = self.dts[k] if self.dts else Cm.T / self.N
                if self.scheme:
                    p = O.make_params(self.m1, self.m2, N, dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, O.EU)
                    out.append(S.solve_one(p, g.Vec_s[k], g.Vec_v[k], g.Delta_s[k], g.Delta_v[k], self.U0[k], self.scheme))
                else:
                    p = O.make_params(self.m1, self.m2, N, dt, self.theta, Cm.R_D, Cm.R_F, *MODEL, Cm.VARIANT[self.variant],
                                      Cm.DIVS if self.div else None, option_type=O.PUT if self.put else O.CALL,
                                      strikes=self.strikes[k] if self.put else None)
                    out.append(O.solve(p, g.Vec_s[k], g.Vec_v[k], g.Delta_s[k], g.Delta_v[k], self.U0[k],
                                       self.U0[k] if "AM" in self.variant else None)[0])
            self._fields[N] = np.stack(out)
        return self._fields[N]


def _words(snaps, n_samp):
    return "sampled ladder: %d snapshots x %d samples" % (len(snaps), n_samp)


def _against_oracle(case, out, snaps, spots, scales=None, v0=None):
    worst = 0.0
    for q, N in enumerate(snaps):
        U = case.fields(N)
        ref, amp, flags = R.sample_batch(U, case.grids.Vec_s, case.grids.Vec_v, case.v0 if v0 is None else v0, spots, scales)
        assert (flags == 0).all()
        bound = 1e-10 * amp * np.abs(U).max(axis=1, keepdims=True)
        diff = np.abs(out[:, q, :] - ref)
        worst = max(worst, (diff / bound).max())
        assert (diff <= bound).all(), (N, np.argwhere(diff > bound)[:4], (diff / bound).max())
    return worst


STREAM, LOOP = "hadi_sample_kernel after each snapshot step", "evaluated inside the time loop"


def _check(sv, case, tuning, names, how, snaps=SNAPS, scales=None):
    """names: what the description of the sample call AND of the ladder call must contain (the same kernels); how: STREAM or LOOP,
    the sample call's own words."""
    with tuned(sv, **tuning):
        out, d = case.samples(sv, snaps, scales=scales)
        assert out.shape == (case.n, len(snaps), case.spots.shape[1])
        assert _words(snaps, case.spots.shape[1]) + (", " if how == STREAM else " ") + how in d and all(x in d for x in names), d
        assert "hadi_sweep_resident" not in d and "hadi_team_kernel" not in d, d
        lad, d1 = case.ladder(sv, snaps)
        assert "maturity ladder" in d1 and all(x in d1 for x in names), d1
        if scales is None:
            assert np.array_equal(out[:, :, 0], lad), out[:, :, 0] - lad
        worst = _against_oracle(case, out, snaps, case.spots, scales)
        print("%s | worst |diff| / bound vs oracle %.2e" % (d[:70], worst))
    return out


# ---- the streaming kernels: one case per layout the packing distinguishes -----------------------------------------------------------
STREAMING = [(50, 25, {}), (100, 30, {}), (200, 20, {}), (300, 20, {"strip": 1}), (300, 20, {"strip": 0}), (600, 12, {}), (1100, 10, {})]


@pytest.mark.parametrize("m1,m2,extra", STREAMING, ids=["%dx%d%s" % (c[0], c[1], "".join("-%s%d" % kv for kv in c[2].items())) for c in STREAMING])
def test_streaming_layouts(solver, m1, m2, extra):
    _check(solver, Case(m1, m2), dict(small_grid=0, **extra), ["row pass"], STREAM)


def test_streaming_scheme_and_scales(solver):
    case = Case(50, 25, scheme=H.SCHEME_MCS, theta=TH_MCS)
    scales = 0.75 + 0.125 * np.arange(case.spots.size).reshape(case.spots.shape)
    _check(solver, case, {"small_grid": 0, "small_sch": 0}, ["row pass", "MCS"], STREAM, scales=scales)


def test_two_streams(solver):
    _check(solver, Case(50, 25, n=4), {"small_grid": 0, "streams": 2}, ["side by side on two streams"], STREAM)


def test_american_on_the_explicit_pair(solver):
    case = Case(50, 25, variant="AM")
    out = _check(solver, case, {"small_grid": 0, "american_p": 1}, ["row pass"], STREAM)
    with tuned(solver, small_grid=0, american_p=1):
        assert "no lambda_bar array" not in case.samples(solver, SNAPS)[1]
    assert np.isfinite(out).all()


# ---- the whole-loop kernels (50x25), through tuning keys -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["EU", "AM"])
def test_block_kernel(solver, variant):
    _check(solver, Case(50, 25, variant=variant), {"small_seq": 0}, ["hadi_small_kernel<"], LOOP)


def test_sequential_kernel(solver):
    _check(solver, Case(50, 25), {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<"], LOOP)


def test_pairs_kernel_with_an_odd_last_instance(solver):
    _check(solver, Case(50, 25), {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<"], LOOP)


@pytest.mark.parametrize("scheme,theta,name", [(H.SCHEME_CRAIG_SNEYD, 0.5, "CS"), (H.SCHEME_MCS, TH_MCS, "MCS"), (H.SCHEME_HV, TH_HV, "HV")],
                         ids=["CS", "MCS", "HV"])
def test_scheme_kernel(solver, scheme, theta, name):
    _check(solver, Case(50, 25, scheme=scheme, theta=theta), {"small_sch": 1},
           ["hadi_small_sch_kernel<1,%s>" % name], LOOP)


def test_dividends_puts_and_per_instance_delta_t(solver):
    _check(solver, Case(50, 25, variant="DIV"), {"small_seq": 1, "small_pairs": 1}, ["hadi_small_seq2_kernel<"], LOOP)
    _check(solver, Case(50, 25, put=True), {"small_seq": 0}, ["hadi_small_kernel<"], LOOP)
    _check(solver, Case(50, 25, dts=[Cm.T / 6, 0.5 / 6, 0.25 / 6]), {"small_seq": 1, "small_pairs": 0}, ["hadi_small_seq_kernel<"], LOOP)


def test_one_list_for_the_batch(solver):
    case = Case(50, 25)
    spots = np.array([Cm.S_0, 3.21, 61.7, 93.3, 101.9, 127.4, 250.3, 519.0, 600.0, 0.011])
    scales = np.linspace(0.8, 1.25, spots.size)
    for tuning in ({"small_seq": 1, "small_pairs": 1}, {"small_grid": 0}):
        with tuned(solver, **tuning):
            out, d = case.samples(solver, SNAPS, spots=spots, scales=scales)
            assert _words(SNAPS, spots.size) in d
            _against_oracle(case, out, SNAPS, spots, scales)


# ---- never the resident sweep, never the team launch ---------------------------------------------------------------------------------
def _excluded(sv, case, snaps, tuning, kernel):
    with tuned(sv, **tuning):
        U = case.U0.copy()
        sv.DO_timestepping(*case.head(), U)
        assert kernel in sv.describe_last_sweep(), sv.describe_last_sweep()
        out, d = case.samples(sv, snaps)
        assert kernel not in d and _words(snaps, case.spots.shape[1]) in d and "hadi_sample_kernel" in d, d
        _against_oracle(case, out, snaps, case.spots)


def test_never_the_resident_sweep(solver):
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the resident sweep's one round of 256 instances needs the 256-CU device")
    _excluded(solver, Case(264, 8, n=256, N=4), [2, 4], {"resident_sweep": 1, "strip": 1}, "hadi_sweep_resident")


def test_never_the_team_launch(solver):
    if solver.device_info()["compute_units"] != 256:
        pytest.skip("the team launch needs the 256-CU device")
    _excluded(solver, Case(200, 16, n=2, N=4), [1, 4], {"team_launch": 1}, "hadi_team_kernel")


# ---- graph cache: the taps are data ------------------------------------------------------------------------------------------------
def test_graph_replays_when_only_the_spots_change(solver):
    case = Case(50, 25)
    snaps = [1, 4, 6]  # (steps no other case of this file uses on this shape: the session's handle has no loop for them yet)
    spots_b = case.spots.copy()
    spots_b[:, 3:8] = 0.5 * (case.spots[:, 3:8] + case.grids.Vec_s[:, 20:25])  # other off-node spots, S_0 kept
    with tuned(solver, small_grid=0, graph=1):
        c0 = Cm.graph_counts(solver)
        a, _ = case.samples(solver, snaps)
        c1 = Cm.graph_counts(solver)
        b, _ = case.samples(solver, snaps, spots=spots_b)
        c2 = Cm.graph_counts(solver)
        a2, _ = case.samples(solver, snaps)
        c3 = Cm.graph_counts(solver)
        d01, d12, d23 = Cm.graph_delta(c0, c1), Cm.graph_delta(c1, c2), Cm.graph_delta(c2, c3)
        assert (d01["captures"], d01["replays"]) == (1, 0), d01
        assert (d12["captures"], d12["replays"], d12["drops"], d12["evictions"]) == (0, 1, 0, 0), d12
        assert (d23["captures"], d23["replays"], d23["drops"], d23["evictions"]) == (0, 1, 0, 0), d23
        assert np.array_equal(a, a2) and not np.array_equal(a[:, :, 3:8], b[:, :, 3:8]) and np.array_equal(a[:, :, 0], b[:, :, 0])
        _against_oracle(case, b, snaps, spots_b)
        # a plain ladder with the same steps is another loop (hadi_snap_kernel), and leaves the sample loop cached
        lad, _ = case.ladder(solver, snaps)
        c4 = Cm.graph_counts(solver)
        assert Cm.graph_delta(c3, c4)["replays"] == 0 and np.array_equal(lad, a[:, :, 0])


# ---- the launchers ---------------------------------------------------------------------------------------------------------------------
def test_base_prices_samples_with_per_instance_v0(solver):
    m1, m2, n, N = 50, 25, 4, 8
    strikes, grids, spots = _batch(m1, m2, n)
    U0 = grids.call_payoff(strikes)
    v0s = [c[1] for c in Cm.mixed_vgrid_candidates(m2, vary_vd=False)][:n]
    per = {"V_0_i": v0s}
    snaps = [1, 5, 8]
    total = (m1 + 1) * (m2 + 1)
    ws = H.DOWorkspace(n, total)
    fields = {}
    for Nq in snaps:  # the oracle on the v-grids rebuilt for each instance's V_0
        p = O.make_params(m1, m2, Nq, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, O.EU)
        vg = [O.rebuild_variance(m2, v) for v in v0s]
        vv, dv = np.stack([x[0] for x in vg]), np.stack([x[1] for x in vg])
        Cm.assert_well_conditioned(grids.Delta_s, dv)
        fields[Nq] = (O.solve_batch(p, grids.Vec_s, vv, grids.Delta_s, dv, U0)[0], vv)
    for tuning, name in (({"small_seq": 0}, "hadi_small_kernel<"), ({"small_grid": 0}, "hadi_sample_kernel")):
        with tuned(solver, **tuning):
            ws.U[...] = U0
            out = solver.compute_base_prices_samples(spots, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, total, N, Cm.THETA, Cm.T / N, n, grids,
                                                     ws, snaps, per_instance=per)
            d = solver.describe_last_sweep()
            assert name in d and _words(snaps, spots.shape[1]) in d, d
            assert np.array_equal(ws.U, U0)  # not written
            lad = solver.compute_base_prices_ladder(Cm.S_0, Cm.V_0, Cm.R_D, Cm.R_F, *MODEL, m1, m2, total, N, Cm.THETA, Cm.T / N, n, grids,
                                                    ws, snaps, per_instance=per)
            assert np.array_equal(out[:, :, 0], lad)
            for q, Nq in enumerate(snaps):
                U, vv = fields[Nq]
                ref, amp, flags = R.sample_batch(U, grids.Vec_s, vv, np.array(v0s), spots)
                assert (flags == 0).all()
                assert (np.abs(out[:, q, :] - ref) <= 1e-10 * amp * np.abs(U).max(axis=1, keepdims=True)).all(), (name, Nq)


def _jac_setup():
    j = Cm.GOLDEN["jacobian"]
    strikes = [float(k) for k in j["strikes"]]
    grids = H.GridViewsBatch.for_strikes(j["m1"], j["m2"], Cm.S_0, Cm.V_0, strikes)
    spots = np.ascontiguousarray(np.stack([R.kernel_test_spots(grids.Vec_s[k], Cm.S_0) for k in range(len(strikes))]))
    return j, strikes, grids, grids.call_payoff(strikes), spots


def test_jacobian_samples_on_a_whole_loop_path_bit_for_bit(solver):
    """Against six sample calls (compute_base_prices_samples: the same v-grid rebuild) with the parameters moved by eps in turn."""
    j, strikes, grids, U0, spots = _jac_setup()
    m1, m2, N, n, eps = j["m1"], j["m2"], j["N"], len(strikes), j["eps"]
    total = (m1 + 1) * (m2 + 1)
    snaps = [5, 12, 20]
    rho, sigma, kappa, eta = MODEL
    with tuned(solver, small_seq=1, small_pairs=0):
        J, base = solver.compute_jacobian_samples(spots, Cm.V_0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, total, N, Cm.THETA,
                                                  Cm.T / N, n, grids, U0, snaps, eps=eps)
        d = solver.describe_last_sweep()
        assert J.shape == (n, 3, spots.shape[1], 5) and base.shape == (n, 3, spots.shape[1])
        assert _words(snaps, spots.shape[1]) in d and "hadi_small_seq_kernel<" in d, d
        ws = H.DOWorkspace(n, total)

        def one(v0, rho, sigma, kappa, eta):
            ws.U[...] = U0
            out = solver.compute_base_prices_samples(spots, v0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, total, N, Cm.THETA,
                                                     Cm.T / N, n, grids, ws, snaps)
            assert "hadi_small_seq_kernel<" in solver.describe_last_sweep()
            return out

        b = one(Cm.V_0, rho, sigma, kappa, eta)
        assert np.array_equal(base, b)
        moved = [one(Cm.V_0, rho, sigma, kappa + eps, eta), one(Cm.V_0, rho, sigma, kappa, eta + eps),
                 one(Cm.V_0, rho, sigma + eps, kappa, eta), one(Cm.V_0, rho + eps, sigma, kappa, eta),
                 one(Cm.V_0 + eps, rho, sigma, kappa, eta)]
        for c, pert in enumerate(moved):
            assert np.array_equal(J[..., c], (pert - b) / eps), c


def test_jacobian_samples_on_the_streaming_path_vs_oracle(solver):
    """The tolerances of the ladder's streaming Jacobian test: prices 1e-9, J 2e-4 (2e-5 on the first three instances); the
    reference is the oracle's own forward differences of sampled fields (v-grids rebuilt for V_0 and V_0 + eps)."""
    j, strikes, grids, U0, spots = _jac_setup()
    m1, m2, N, n, eps = j["m1"], j["m2"], j["N"], len(strikes), j["eps"]
    snaps = [5, 12, 20]
    rho, sigma, kappa, eta = MODEL
    with tuned(solver, small_grid=0):
        J, base = solver.compute_jacobian_samples(spots, Cm.V_0, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, m1, m2, (m1 + 1) * (m2 + 1), N,
                                                  Cm.THETA, Cm.T / N, n, grids, U0, snaps, eps=eps)
        assert "hadi_sample_kernel" in solver.describe_last_sweep()

    def ref(Nq, v0, rho, sigma, kappa, eta):
        vv, dv = O.rebuild_variance(m2, v0)
        p = O.make_params(m1, m2, Nq, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, rho, sigma, kappa, eta, O.EU)
        U = O.solve_batch(p, grids.Vec_s, np.tile(vv, (n, 1)), grids.Delta_s, np.tile(dv, (n, 1)), U0)[0]
        return R.sample_batch(U, grids.Vec_s, np.tile(vv, (n, 1)), v0, spots)[0]

    for q, Nq in enumerate(snaps):
        b = ref(Nq, Cm.V_0, rho, sigma, kappa, eta)
        moved = [ref(Nq, Cm.V_0, rho, sigma, kappa + eps, eta), ref(Nq, Cm.V_0, rho, sigma, kappa, eta + eps),
                 ref(Nq, Cm.V_0, rho, sigma + eps, kappa, eta), ref(Nq, Cm.V_0, rho + eps, sigma, kappa, eta),
                 ref(Nq, Cm.V_0 + eps, rho, sigma, kappa, eta)]
        Jo = np.stack([(m - b) / eps for m in moved], axis=-1)
        assert np.abs(base[:, q] - b).max() <= 1e-9
        assert np.abs(J[:, q] - Jo).max() <= 2e-4 and np.abs(J[:3, q] - Jo[:3]).max() <= 2e-5, Nq
    assert abs(base[0, 2, 0] - j["base_price_0"]) <= 1e-9  # the row the reference printed: the S_0 column at the ladder's top


def test_device_memory_outputs(solver):
    import torch
    case = Case(50, 25)
    host, _ = case.samples(solver, [2, 6])
    dev = torch.device("cuda", 0)
    g = case.grids.to(dev)
    U = torch.from_numpy(case.U0.copy()).to(dev)
    out = solver.sample_ladder(*case.head()[:-1], g, U, case.spots, case.v0, [2, 6])
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), host)
    assert np.array_equal(U.cpu().numpy(), case.U0)


def test_surface_end_to_end_through_strike_samples(solver):
    """A 100x50 surface of 7 strikes x 3 maturities from ONE instance built at K = 100."""
    m1, m2, N, K = 100, 50, 12, 100.0
    strikes = [85.0, 90.0, 95.0, 100.0, 105.0, 112.5, 120.0]
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, [K])
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff([K])
    spots, scales = H.strike_samples(Cm.S_0, K, strikes)
    snaps = [4, 8, 12]
    out = solver.sample_ladder(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, grids, U0.copy(), spots, Cm.V_0, snaps, scales=scales)
    assert out.shape == (1, 3, 7) and _words(snaps, 7) in solver.describe_last_sweep()
    for q, Nq in enumerate(snaps):
        p = O.make_params(m1, m2, Nq, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, O.EU)
        U = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0)[0]
        ref, amp, flags = R.sample_batch(U, grids.Vec_s, grids.Vec_v, Cm.V_0, spots, scales)
        assert (flags == 0).all() and (np.abs(out[:, q] - ref) <= 1e-10 * amp * np.abs(U).max()).all(), Nq
    assert (np.diff(out[0], axis=1) < 0).all() and (np.diff(out[0], axis=0) > 0).all()  # calls: falling in K, rising in T (r_f = 0)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def _status(fn, *a, **kw):
    with pytest.raises(H.HadiError) as e:
        fn(*a, **kw)
    return e.value.status


def test_errors(solver):
    INVALID, UNSUPPORTED, NOT_ON_GRID = 1, 2, 4
    case = Case(50, 25)
    head, U0, sp = case.head(), case.U0, case.spots
    call = solver.sample_ladder
    # every refusal of the ladder keeps its status
    for bad in ([0, 3], [3, 3], [4, 2], [7], [1, 2, 3, 4, 5, 6, 7], [-1]):
        assert _status(call, *head, U0.copy(), sp, case.v0, bad) == INVALID, bad
    assert _status(call, *head, U0.copy(), sp, case.v0, [2], per_instance={"N_i": [6, 6, 6]}) == INVALID
    assert _status(call, *head, U0.copy(), sp, case.v0, [2], variant=H.AM, U_0=U0, scheme=H.SCHEME_MCS) == UNSUPPORTED
    h7 = head[:6] + (0.007,) + head[7:]
    assert _status(call, *h7, U0.copy(), sp, case.v0, [2]) == UNSUPPORTED  # call data with r_f != 0
    assert call(*h7, Cm.put_payoff(case.grids.Vec_s, case.strikes, 25), sp, case.v0, [2], option_type=H.PUT, strikes=case.strikes).shape == (3, 1, 10)
    assert call(*head, U0.copy(), sp, 0.0123456, [2]).shape == (3, 1, 10)  # V_0 off the v-grid: row 0, as the price pick
    # off the s-grid: NaN in that entry, the others valid
    good = call(*head, U0.copy(), sp, case.v0, [2, 6])
    for x in (case.grids.Vec_s[1, 0] - 1e-3, case.grids.Vec_s[1, -1] + 1e-3, np.nan):
        off = sp.copy()
        off[1, 4] = x
        assert _status(call, *head, U0.copy(), off, case.v0, [2, 6]) == NOT_ON_GRID, x
    # the raw ABI: the struct's own refusals, NULL outputs, the fp32 state, a degenerate stencil
    steps = np.array([2, 6], dtype=np.int32)
    stp = steps.ctypes.data_as(C.POINTER(C.c_int))
    out = np.zeros((3, 2, 10))
    optr = C.c_void_p(out.ctypes.data)
    Jb = np.zeros((3, 2, 10, 5))
    lib, h = solver._lib, solver._h
    p = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy())
    dp = lambda a: a.ctypes.data_as(nat._dp)
    sc = np.ones_like(sp)
    ok = nat.Samples(10, dp(sp), None, 3)
    run = lambda st, o=optr: lib.hadi_sample_ladder(h, C.byref(p), case.v0, C.byref(st) if st is not None else None, 2, stp, o)
    assert run(None) == INVALID and run(ok, None) == INVALID
    assert run(nat.Samples(10, None, None, 3)) == INVALID
    assert run(nat.Samples(0, dp(sp), None, 3)) == INVALID and run(nat.Samples(1025, dp(sp), None, 3)) == INVALID
    assert run(nat.Samples(10, dp(sp), None, 2)) == INVALID and run(nat.Samples(10, dp(sp), None, 0)) == INVALID
    for badscale in (np.inf, np.nan):
        sc[2, 5] = badscale
        assert run(nat.Samples(10, dp(sp), dp(sc), 3)) == INVALID
    assert lib.hadi_sample_ladder(h, C.byref(p), case.v0, C.byref(ok), 2, None, optr) == INVALID
    assert lib.hadi_compute_base_prices_samples(h, C.byref(p), case.v0, C.byref(ok), 2, stp, None) == INVALID
    pj = solver._problem(H.EU, *head[:11], case.grids, U_0=U0.copy(), need_vgrid=False)
    assert lib.hadi_compute_jacobian_samples(h, C.byref(pj), case.v0, 1e-6, C.byref(ok), 2, stp, None, optr) == INVALID
    assert lib.hadi_compute_jacobian_samples(h, C.byref(pj), case.v0, 1e-6, C.byref(ok), 2, stp, C.c_void_p(Jb.ctypes.data), None) == INVALID
    assert lib.hadi_compute_jacobian_samples(h, C.byref(pj), case.v0, 1e-6, None, 2, stp, C.c_void_p(Jb.ctypes.data), optr) == INVALID
    p32 = solver._problem(H.EU, *head[:11], case.grids, U=U0.copy(), state_precision=nat.STATE_FP32)
    assert lib.hadi_sample_ladder(h, C.byref(p32), case.v0, C.byref(ok), 2, stp, optr) == UNSUPPORTED
    # a stencil with a zero interval: HADI_ERR_INVALID (the grid is only read by the locate kernel before the sweep refuses nothing)
    g2 = Cm.spot_scaled_grids(case.grids, 0)
    g2.Vec_s = case.grids.Vec_s.copy()
    g2.Vec_s[0, 31] = g2.Vec_s[0, 30]
    deg = sp.copy()
    deg[0, 3] = 0.5 * (g2.Vec_s[0, 31] + g2.Vec_s[0, 32])
    hd = head[:-1] + (g2,)
    assert _status(call, *hd, U0.copy(), deg, case.v0, [2]) == INVALID
    # and the handle still works: the off-grid entry alone is NaN, the call's other entries are those of the good call
    off = sp.copy()
    off[1, 4] = np.nan
    st = nat.Samples(10, dp(off), None, 3)
    assert run(st) == NOT_ON_GRID
    bad = np.zeros(out.shape, dtype=bool)
    bad[1, :, 4] = True
    assert np.isnan(out[bad]).all() and np.array_equal(out[~bad], good[~bad])
    assert run(ok) == 0 and np.array_equal(out, good)
