"""Theta and time-step regimes shared by the CPU and GPU time-regime tests (test_oracle_time_regimes.py,
test_emu_time_regimes.py, test_gpu_time_regimes.py), the rotation that puts several (delta_t_i, N_i) into one batch, and the
dividend schedule of a regime.

The rest of the suite runs theta = 0.8 with dt = T / N = 1 / N almost throughout.  Theta and dt select code paths and
conditioning (hadi_core.h: thdt = theta dt, RC_VTH = thdt v, a2i = I - theta dt A2, the strips' A0 weights divided by
-theta dt (r_d - r_f); hadi_route.h: strips, team kernel and resident sweep off at theta == 0): a large theta dt puts every line
system far from the identity (un-pivoted pentadiagonal LU, the SPIKE reduced system, the Newton-refined reciprocal), theta dt -> 0
makes the implicit stage the identity while lambda_bar = (U0 - P) / dt amplifies round-off by 1 / dt."""
import common as Cm
import dividend_schedules as D

CANONICAL_THETA = Cm.THETA

# dt = None: T / N of the case; N = None: the N of the row that runs the regime.  lambda_xp: the worst distance of the fp64
# oracle's lambda_bar from its binary128 twin, relative to max(1, max|lambda|), that tests/test_oracle_time_regimes.py measures
# and prints over its shapes (it asserts that no measurement exceeds the entry): the reference's own error, from which the GPU
# bound on lambda_bar follows (lambda_bound).  DIV: whether the dividend rows run the regime.
#         id    theta  dt     N     lambda_xp  DIV    what it reaches
TIMES = [("T0", 0.5,   None,  None, 1.0e-11,   True),   # Crank-Nicolson weights
         ("T1", 1.0,   None,  None, 8.4e-12,   True),   # fully implicit: the explicit share of A1 / A2 vanishes
         ("T2", 2.0,   None,  None, 5.6e-12,   True),   # over-implicit, negative explicit share (accepted by the API)
         ("T3", 0.0,   1e-4,  1,    8.8e-10,   False),  # explicit: a2i is the identity; strips, team kernel and resident sweep OFF.
                                                        # One step only (more are unstable on the fine grids).  No DIV: with N = 1
                                                        # a date is paid only inside [dt, 2 dt), which no fraction of N dt reaches
         ("T4", 0.8,   5.0,   3,    2.6e-12,   True),   # theta dt = 4: line systems far from I
         ("T5", 1.0,   50.0,  2,    7.6e-13,   True),   # theta dt = 50
         ("T6", 0.8,   1e-6,  3,    3.8e-8,    True),   # implicit stage close to I; lambda_bar amplified by 1 / dt
         ("T7", 1e-9,  1e-6,  3,    4.9e-8,    True)]   # theta tiny but positive: strips stay ON, A0 weights / (theta dt q) ~ 7e16
TIME = {t[0]: t[1:] for t in TIMES}
TIME_IDS = [t[0] for t in TIMES]
EXPLICIT = ("T3",)               # theta == 0: hadi_no_strips, hadi_team_grid and hadi_resident_grid refuse
FP32_IDS = ("T0", "T1", "T2", "T4")  # (in the tiny-dt regimes the whole step is below an fp32 ulp: rounding ties, not a check)
SMALL_DT = ("T3", "T6", "T7")    # lambda_bar's round-off is the field's divided by dt
# Dividend cases: the dating rule (dividend_schedules.py) pays a date of the canonical fractions 0.2 .. 0.8 of the horizon only
# with five steps or more, so where the regime's N (fixed, or the row's own) is below 5 a dividend case keeps the regime's theta
# and dt and takes N_DIV steps.
N_DIV = 10
# T7 differs from T6 in theta alone.  On coarse s-grids three steps of 1e-6 are so nearly the identity that theta does not show:
# European call data, |U(T7) - U(T6)| / max|U|: 50x25 6.9e-8, 40x600 1.1e-7, 50x300 1.2e-7, 100x20 5.8e-7, 100x50 8.7e-7 -- below
# the 1e-6 a regime must move the field by, so the GPU rows on those shapes do not run T7 (a kernel that used theta 0.8 there
# could pass).  From 128x64 on it is 2.3e-6 .. 3.9e-4 (test_oracle_time_regimes.py asserts both lists).
T7_DROPPED = [(50, 25), (40, 600), (50, 300), (100, 20), (100, 50)]
T7_SHAPES = [(128, 64), (200, 60), (300, 80), (300, 140), (256, 128), (300, 264), (600, 40), (1100, 20)]
ADJUDICATION_MARGIN = 30.0      # ADVICE.md / tools/fuzz_parity.py: a bound is 30x the reference's own error
LAMBDA_FLOOR = 1e-8              # the project's lambda_bar bound, relative to max(1, max|lambda|)


def regime(tid, N_row, dividends=False):
    """(theta, dt, N) of regime `tid` for a row whose own N is N_row."""
    theta, dt, N = TIME[tid][:3]
    N = N_row if N is None else N
    if dividends and N < 5:
        N = N_DIV
    return theta, (Cm.T / N if dt is None else dt), N


def canonical(N):
    """The canonical-time point a regime is held against: theta 0.8, dt = T / N, the same N."""
    return CANONICAL_THETA, Cm.T / N, N


def lambda_bound(tid):
    """The bound on lambda_bar, relative to max(1, max|lambda|): 30x the oracle's own distance from its twin, never below the
    project's 1e-8."""
    return max(LAMBDA_FLOOR, ADJUDICATION_MARGIN * TIME[tid][3])


def has_dividends(tid):
    return TIME[tid][4]


def runs(tid, m1, m2, dividends=False, fp32=False):
    """Whether a GPU row on an m1 x m2 grid runs regime `tid` (the three exclusions of the table above)."""
    if dividends and not has_dividends(tid):
        return False
    if fp32 and tid not in FP32_IDS:
        return False
    return tid != "T7" or (m1, m2) not in T7_DROPPED


# Theta is a scalar of the ABI, so a rotated batch shares one theta (0.8) and rotates (delta_t_i, N_i).
#            dt          N
ROTATION = [(5.0,        3),   # T4
            (1e-6,       3),   # T6
            (Cm.T / 4,   4),   # canonical
            (1e-3,       2)]
ROTATION_LAMBDA = lambda_bound("T6")  # (a rotated American batch holds a dt = 1e-6 instance)


def time_rotation(n, c=0):
    """Instance k of a batch takes the (dt, N) of ROTATION[(k + c) % 4]: neighbours never share a dt; [n] tuples (dt, N)."""
    return [ROTATION[(k + c) % len(ROTATION)] for k in range(n)]


def per_instance(times):
    """The delta_t_i / N_i of the C ABI for a list of (dt, N)."""
    return {"delta_t_i": [t[0] for t in times], "N_i": [t[1] for t in times]}


def dividends_at(N, dt, divs=Cm.DIVS):
    """The canonical schedule with its dates at the same fractions of the horizon N dt (amounts and percentages stay).  Asserts
    with the dating mirror that at least one dividend is paid."""
    dates = [d / Cm.T * (N * dt) for d in divs[0]]
    paid = D.paying_steps(N, dt, dates)
    assert paid, "no dividend of %r is paid on %d steps of %r" % (dates, N, dt)
    return dates, list(divs[1]), list(divs[2])
