"""The domain of the whole-loop Bates kernel, hadi_small_jump_kernel<B, W>, as one table for the CPU tests
(tests/test_emu_bates_samples.py, tests/test_emu_small_jump_stage.py) and the device tests (tests/test_gpu_bates_sample_domain.py).
Plain data and numpy.

SHAPES.  The jump stage (hadi_small_jump_stage, csrc/hadi_k_small.h) deals ceil(nrows / 16) * nib accumulator tiles of 16 v-rows x 16
slots round-robin over W = 4 or 8 wavefronts, nrows = m2 + 1, nib = ceil(rowp / 16), rowp = 64 B + 8, and masks rows >= nrows, slots
past the pitch and slots that hold no node.  The rows: event_cases.LDS_ROWS, 50x32, 100x12 and 128 x the largest m2 the route admits,
which the caller FINDS (largest_m2 below with the emulator's route function or the device's description) and never writes down.
what(row) is the sentence of a row: tiles against W, rows in the last row block, node slots of 64 B.

Grids are Cm.well_conditioned_strikes with Cm.assert_well_conditioned -- asserted, never a filter.  Laws cycle through five
(lambda, mu_J, sigma_J), the third with lambda = 0.  Spots and scales are sample_cases.batch_spots with a budget of 64 unless a test
says otherwise: scales other than 1, node hits and tolerance hits in every call.

Bounds, the project's own (nothing is measured here):
  samples        |out - ref| <= 1e-10 sum|w| |scale| max|U_ref|                                   (within_bound)
  interior       against the node-hit columns of the same call: sample_cases.tight_check
  base samples   1e-10 relative, J per column 2e-4 sum|w| |scale| with eps = 1e-6                  (jacobian_within_bounds)
                 -- stated by the project for rows of at most 100 nodes, so the Jacobian cases are JAC_SHAPES: 50x25 and, for
                 B = 2, 96x12 (assert_well_conditioned accepts it; asserted where it is used).
The reference is tests/bates_samples_ref.py on the DISTINCT instances only, computed once per (batch, schedule) and kept."""
import collections

import numpy as np

import bates_samples_ref as BS
import common as Cm
import event_cases as EC
import sample_cases as SC

MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
EPS = 1e-6
WIDTHS = (4, 8)
BUDGET = 64
# per-instance jump laws, cycled through a batch; the third has intensity 0
LAM, MU, SIG = (0.5, 2.0, 0.0, 1.0, 0.3), (-0.10, -0.05, 0.05, -0.20, 0.10), (0.15, 0.10, 0.20, 0.25, 0.30)

Row = collections.namedtuple("Row", "m1 m2 why")
_WHY = {(16, 11): "fewer tiles than wavefronts at W = 8; rows that are mostly empty",
        (63, 24): "an odd number of nodes, one slot short of full; two row blocks",
        (64, 31): "rows that are exactly full (B = 1); two row blocks exactly full",
        (64, 32): "rows that are exactly full (B = 1); 33 v-rows, a last row block of a single row",
        (127, 16): "B = 2, one slot short of full; 17 v-rows, a last row block of a single row",
        (128, 20): "rows that are exactly full (B = 2)",
        (50, 32): "the calibration width with 33 v-rows: a last row block of a single row",
        (100, 12): "B = 2 with 13 v-rows: one row block of nine tiles, so one wavefront of eight takes two"}
FIXED = [Row(m1, m2, _WHY[(m1, m2)]) for m1, m2 in list(EC.LDS_ROWS) + [(50, 32), (100, 12)]]
LARGEST_M1 = 128
JAC_SHAPES = ((50, 25), (96, 12))


def laws(n, first=0):
    return tuple(np.array([x[(first + k) % 5] for k in range(n)]) for x in (LAM, MU, SIG))


def geometry(m1, m2):
    """(B, rowp, nib, row blocks, tiles, rows in the last row block) of the stage on a shape."""
    B = EC.pick_shape(m1)[0]
    rowp, nrows = 64 * B + 8, m2 + 1
    nib, rb = (rowp + 15) // 16, (nrows + 15) // 16
    return B, rowp, nib, rb, rb * nib, nrows - 16 * (rb - 1)


def what(row):
    B, rowp, nib, rb, tiles, last = geometry(row.m1, row.m2)
    return "%dx%d: %d tiles (row blocks %d x slot blocks %d) over W = 4 / 8 -> at most %d / %d per wavefront%s; rows in the last row " \
           "block: %d; %d of %d slots hold a node (+ i = 0 at slot %d of pitch %d) -- %s" % (
               row.m1, row.m2, tiles, rb, nib, -(-tiles // 4), -(-tiles // 8), ", %d wavefronts idle at W = 8" % (8 - tiles) if tiles < 8 else "",
               last, row.m1, 64 * B, 64 * B, rowp, row.why)


def largest_m2(takes_the_loop, m1=LARGEST_M1, start=20):
    """The largest m2 at which takes_the_loop(m1, m2) -- the emulator's route function, or a device call's description -- still says
    hadi_small_jump_kernel<2,..>; found by walking up from an LDS_ROWS shape, never hard-coded.  (m2 + 1 streams: the caller asserts
    the words it sees there.)"""
    assert (m1, start) in EC.LDS_ROWS and takes_the_loop(m1, start)
    m2 = start
    while takes_the_loop(m1, m2 + 1):
        m2 += 1
        assert m2 < 64
    return m2


def shapes(m2_max):
    """Every row of the table, the found one last."""
    return FIXED + [Row(LARGEST_M1, m2_max, "the largest B = 2 instance the 76 KiB LDS limit admits (m2 found at run time)")]


def row_id(r):
    return "%dx%d" % (r[0], r[1])


# ---- batches ------------------------------------------------------------------------------------------------------------------------
class Distinct:
    """d DIFFERENT instances of one shape: strike, grid, payoff, law and sample list each their own; built once, left unchanged.
    make_grids(m1, m2, strikes, V_0) -> (Vec_s, Vec_v, Delta_s, Delta_v, call payoff): Cm.oracle_grids, or the package's builder."""

    def __init__(self, m1, m2, d, put=False, first=0, budget=BUDGET, count=None, make_grids=None, same=False):
        self.m1, self.m2, self.d, self.put, self.V_0 = m1, m2, d, put, Cm.v0_for(m2)
        # (same: one strike and grid for all d -- the batch of a shared-grid call; the laws still differ)
        self.strikes = np.array(Cm.well_conditioned_strikes(m1, 1) * d if same else Cm.well_conditioned_strikes(m1, d))
        self.vs, self.vv, self.ds, self.dv, call = (make_grids or (lambda *a: Cm.oracle_grids(a[0], a[1], a[2], V0=a[3])))(
            m1, m2, list(self.strikes), self.V_0)
        Cm.assert_well_conditioned(self.ds, self.dv)
        self.U0 = Cm.put_payoff(self.vs, self.strikes, m2) if put else np.ascontiguousarray(call)
        self.lam, self.mu, self.sig = laws(d, first)
        self.spots, self.scales, self.kinds = SC.batch_spots(self.vs, Cm.S_0, budget, count)
        assert (self.spots[:, 0] == Cm.S_0).all() and (count == 1 or ((self.scales != 1.0).any() and (self.kinds == SC.HIT).any()))
        for a in (self.vs, self.vv, self.ds, self.dv, self.U0, self.lam, self.mu, self.sig, self.strikes):
            a.setflags(write=False)
        self._ref = {}

    def fields(self):
        return dict(strikes=self.strikes, vs=self.vs, vv=self.vv, ds=self.ds, dv=self.dv, U0=self.U0, lam=self.lam, mu=self.mu,
                    sig=self.sig, spots=self.spots, scales=self.scales)

    def ref(self, N, snaps, law=None, div=False, dts=None):
        """bates_samples_ref.sample_ladder's (values, sum|w| |scale|, max|U|) of the d instances; dts: delta_t of each of them."""
        law = (self.lam, self.mu, self.sig) if law is None else tuple(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.d,)) for x in law)
        key = (N, tuple(snaps), div, None if dts is None else tuple(dts)) + tuple(x.tobytes() for x in law)
        if key not in self._ref:
            self._ref[key] = BS.sample_ladder(self.m1, self.m2, list(snaps), Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, self.vs, self.vv,
                                              self.ds, self.dv, self.U0, self.V_0, self.spots, self.scales, *law,
                                              dividends=Cm.DIVS if div else None, put_strikes=self.strikes if self.put else None,
                                              dt_i=None if dts is None else list(dts))
        return self._ref[key]

    def ref_jacobian(self, N, snaps, n_par):
        key = ("J", N, tuple(snaps), n_par)
        if key not in self._ref:
            self._ref[key] = BS.jacobian(self.m1, self.m2, list(snaps), Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, *MODEL, self.V_0, self.vs, self.ds,
                                         self.U0, self.spots, self.scales, self.lam, self.mu, self.sig, n_par=n_par, eps=EPS,
                                         put_strikes=self.strikes if self.put else None)
        return self._ref[key]


_DISTINCT = {}


def distinct(m1, m2, d, **kw):
    key = (m1, m2, d) + tuple(sorted((k, v if not callable(v) else id(v)) for k, v in kw.items()))
    if key not in _DISTINCT:
        _DISTINCT[key] = Distinct(m1, m2, d, **kw)
    return _DISTINCT[key]


def replicated(dist, n):
    """A batch of n instances that cycles over the d of `dist`: strike, grid, payoff, law (lambda, mu_J, sigma_J) and spots of
    instance k are those of k % d.  Returns (the batch's arrays by name, the index of every instance's first twin)."""
    fields = dist.fields() if isinstance(dist, Distinct) else dist
    d = len(fields["strikes"])
    twin = np.arange(n) % d
    assert n >= d and (np.asarray(fields["lam"]) == 0.0).any(), "one distinct instance has lambda = 0"
    return {k: np.ascontiguousarray(np.asarray(v)[twin]) for k, v in fields.items()}, twin


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
WORST = {"samples": 0.0, "tight": 0.0, "base": 0.0, "J": 0.0}


def within_bound(name, out, ref):
    vals, amp, top = ref
    bound = 1e-10 * amp * top[:, :, None]
    worst = float((np.abs(out - vals) / bound).max())
    WORST["samples"] = max(WORST["samples"], worst)
    print("%s: worst |diff| / bound %.2e (file so far %.2e)" % (name, worst, WORST["samples"]))
    assert np.isfinite(out).all() and worst <= 1.0, (name, worst)
    return worst


def tight(name, out, vs, spots, scales, kinds):
    worst, checked = SC.tight_check(out, vs, spots, scales, name)
    assert checked == int(((kinds == SC.INTERIOR) | (kinds == SC.TOL_INTERIOR)).sum())
    WORST["tight"] = max(WORST["tight"], worst)
    print("%s: tight check %.3f of its bound over %d interior samples (file so far %.3f)" % (name, worst, checked, WORST["tight"]))
    return worst


def jacobian_within_bounds(name, J, base, Jo, bo, amp):
    rel = np.abs(base - bo) / np.maximum(1.0, np.abs(bo))
    dj = (np.abs(J - Jo) / amp[..., None]).reshape(-1, J.shape[-1]).max(axis=0)
    WORST["base"], WORST["J"] = max(WORST["base"], float(rel.max()) / 1e-10), max(WORST["J"], float(dj.max()) / 2e-4)
    print("%s: base %.2e relative, J per column / (sum|w| |scale|) %s (file so far: %.3f and %.3f of the bounds)"
          % (name, rel.max(), " ".join("%.1e" % x for x in dj), WORST["base"], WORST["J"]))
    assert np.isfinite(J).all() and rel.max() <= 1e-10 and dj.max() <= 2e-4, (name, rel.max(), dj)
