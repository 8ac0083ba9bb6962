"""Dividend schedules for the jump kernels and the host routine that dates them (hadi_plan.h, hadi_dividend_steps), shared
by the emulator tests (tests/test_emu_dividends.py) and the GPU tests (tests/test_gpu_dividends.py).

The dating rule, as hadi_plan.h states it and as include/hadi.h documents it at hadi_problem's dividend fields: the dates are
consumed in ARRAY order by one running index; at step n = 1..N the dividend under the index is paid when
n*dt <= date < (n+1)*dt (both products in fp64), and AFTERWARDS the index advances by one if n*dt > date.  So a date before dt
is never paid, of two dates inside one step interval the second is skipped, the index moves at most one place per step (a
cluster of dates makes it lag behind later ones), and -- because the index only leaves a paid date on the FOLLOWING step, where
it then points at the next date for the first time one step later still -- two paying steps are never adjacent: the densest
schedule the rule admits pays on every other step.  `paying_steps` is that rule in plain Python; `branch_counts` says which
branch of the jump's interpolation every s-node of a paying step takes.  Tests assert with the two that a schedule reaches the
branch it is named for on the grid they use."""
import collections
import random

import numpy as np

EPS = 1e-12  # relative nudge that puts a date just inside the step interval it is meant for


def named(N, dt, T):
    """name -> (dates, amounts, percentages) for a sweep of N steps of dt (T is the maturity the dates are scaled to)."""
    eps = 1.0 + EPS
    half = max(3, N // 2)
    s = collections.OrderedDict()
    # the suite's fixture (tests/golden/reference_known_answers.json), scaled to T: four small, well-separated payments
    s["canon"] = ([0.2 * T, 0.4 * T, 0.6 * T, 0.8 * T], [0.5, 0.3, 0.2, 0.1], [0.02] * 4)
    # a date before dt is never paid (step 1 already has dt > date); the index moves on and the second date is paid on step 3
    s["before_dt"] = ([0.5 * dt, 3.5 * dt], [1.0, 0.7], [0.01, 0.02])
    # a jump at the start of step 1: on the initial condition, and on the American step that is explicit anyway
    s["step1"] = ([1.5 * dt, (half + 0.5) * dt], [1.0, 0.5], [0.02, 0.01])
    # a jump at the start of the LAST step (date in [N dt, (N+1) dt), i.e. at or after T)
    s["lastN"] = ([2.5 * dt, (N + 0.5) * dt], [0.5, 1.0], [0.01, 0.02])
    # dates from (N+1) dt on are never paid
    s["beyondT"] = ([2.5 * dt, (N + 1.5) * dt, (N + 5) * dt], [0.8, 50.0, 50.0], [0.01, 0.5, 0.5])
    # two dates inside step 2's interval: the second is skipped (and would show: it is large); the third is paid on step 5
    s["same_step"] = ([2.2 * dt, 2.7 * dt, 5.5 * dt], [0.6, 40.0, 0.4], [0.01, 0.3, 0.02])
    # four dates inside step 1's interval, then one at 4.5 dt: the index advances one place per step, reaches the fifth date on
    # step 6 and never pays it
    s["cluster"] = ([1.1 * dt, 1.3 * dt, 1.5 * dt, 1.7 * dt, 4.5 * dt], [0.5, 30.0, 30.0, 30.0, 30.0], [0.01, 0.2, 0.2, 0.2, 0.2])
    # array order, not date order: the index waits at 5.5 dt, pays it, then finds 2.5 dt in the past and drops it, pays 8.5 dt
    s["unsorted"] = ([5.5 * dt, 2.5 * dt, 8.5 * dt], [0.5, 35.0, 0.7], [0.01, 0.3, 0.02])
    # 60 on a spot of 100: a band of low nodes has ex-dividend spot <= 0 (call -> 0, put -> its s = 0 value), the rest interpolate
    s["big_cash"] = ([2.5 * dt], [60.0], [0.0])
    # every node has ex-dividend spot <= 0
    s["huge_cash"] = ([2.5 * dt], [1e4], [0.0])
    # proportional dividends only
    s["pct_only"] = ([2.5 * dt, 5.5 * dt], [0.0, 0.0], [0.1, 0.5])
    # percentage 1.0: every node lands on ex-dividend spot 0 exactly, which counts as <= 0
    s["pct_one"] = ([2.5 * dt], [0.0], [1.0])
    # a zero dividend is not the identity: node m1 finds no s_k > new_s and takes node 0's value (the reference's idx == 0 quirk)
    s["zero"] = ([2.5 * dt], [0.0], [0.0])
    # a negative amount lifts the top nodes above s_max: same fallback branch
    s["negative"] = ([2.5 * dt, 5.5 * dt], [-5.0, -0.5], [0.0, 0.0])
    # a date just inside every step's interval: the rule pays the first and lags one step behind all the others
    s["every_step"] = ([k * dt * eps for k in range(1, N + 1)], [0.3] * N, [0.01] * N)
    # the same with dates that are exactly the products k*dt the rule compares with (k*dt <= date holds with equality)
    s["on_grid"] = ([k * dt for k in range(1, N + 1)], [0.3] * N, [0.01] * N)
    # the densest schedule the rule admits: a date just inside every ODD step's interval, each one paid
    s["alternate"] = ([k * dt * eps for k in range(1, N + 1, 2)], [0.3] * ((N + 1) // 2), [0.01] * ((N + 1) // 2))
    # ... and with dates exactly on the odd multiples of dt: paid by equality on every one of those steps
    s["on_grid_odd"] = ([k * dt for k in range(1, N + 1, 2)], [0.3] * ((N + 1) // 2), [0.01] * ((N + 1) // 2))
    # dividend variant with num_dividends = 0: no jump, the plain sweep
    s["empty"] = ([], [], [])
    return s


NAMES = list(named(10, 0.1, 1.0))


def random_schedule(rng, N, dt):
    """0 .. 2N dividends from a random.Random: dates in [0, 1.3 N dt], three in ten snapped to exact multiples of dt, three
    schedules in ten left unsorted; amounts in [-2, 80] (mostly a few units, now and then large or negative), percentages in
    [0, 1] (mostly a few per cent, now and then up to 1)."""
    nd = rng.randint(0, 2 * N)
    dates, amounts, pcts = [], [], []
    for _ in range(nd):
        d = rng.uniform(0.0, 1.3 * N * dt)
        if rng.random() < 0.3:
            d = round(d / dt) * dt
        dates.append(d)
        u = rng.random()
        amounts.append(rng.uniform(0.0, 3.0) if u < 0.7 else rng.uniform(3.0, 80.0) if u < 0.85 else rng.uniform(-2.0, 0.0) if u < 0.95 else 0.0)
        u = rng.random()
        pcts.append(rng.uniform(0.0, 0.05) if u < 0.7 else rng.uniform(0.05, 1.0) if u < 0.9 else 0.0 if u < 0.97 else 1.0)
    if rng.random() >= 0.3:
        dates.sort()
    return dates, amounts, pcts


def paying_steps(N, dt, dates):
    """{step n: index of the dividend paid at the start of step n}, by the rule in this module's docstring.  The rule is three
    comparisons and one running index, so this is a second transcription of it beside hadi_dividend_steps, not an independent
    derivation: the dating tests guard the host routine against edits and check its table layout (len > N, -1 entries); the
    independent check of the dating is the oracle's own loop, in the field tests."""
    paid, k = {}, 0
    for n in range(1, N + 1):
        if k >= len(dates):
            break
        t, t_next, date = n * dt, (n + 1) * dt, dates[k]
        if t <= date and date < t_next:
            paid[n] = k
        if t > date:
            k += 1
    return paid


def flags(N, dt, dates, length=None):
    """paying_steps as the table hadi_dividend_steps fills: entry n-1 is the index paid at step n or -1; -1 beyond N."""
    out = [-1] * (N if length is None else length)
    for n, k in paying_steps(N, dt, dates).items():
        out[n - 1] = k
    return out


Branches = collections.namedtuple("Branches", "nonpos interior fallback below_s0")


def branch_counts(vec_s, schedule, paid):
    """{step n: Branches} for the paying steps `paid` (from paying_steps): how many s-nodes have ex-dividend spot
    new_s = s (1 - pct) - amount <= 0, how many interpolate between two nodes, how many find no node above new_s or have
    new_s below node 0 and take node 0's value (fallback), and how many of the latter are the 0 < new_s < s_0 kind."""
    vec_s = np.asarray(vec_s, dtype=np.float64)
    _, amounts, pcts = schedule
    out = {}
    for n, k in sorted(paid.items()):
        new_s = vec_s * (1.0 - pcts[k]) - amounts[k]
        pos = new_s > 0
        idx = np.searchsorted(vec_s, new_s, side="right")  # first node strictly above new_s; len(vec_s) if there is none
        fb = pos & ((idx == 0) | (idx == len(vec_s)))
        out[n] = Branches(int((~pos).sum()), int((pos & ~fb).sum()), int(fb.sum()), int((pos & (idx == 0)).sum()))
    return out


def total(counts):
    """Branches summed over the paying steps."""
    return Branches(*(sum(c[f] for c in counts.values()) for f in range(4)))


def requirement(name, N, dt, schedule, vec_s):
    """Asserts that `schedule` (the one called `name`) reaches the branch it exists for with N steps of dt on the s-grid vec_s;
    returns (paid, counts).  Conditions on the INPUTS, computed on the host -- never on what a kernel returned."""
    dates = schedule[0]
    paid = paying_steps(N, dt, dates)
    counts = branch_counts(vec_s, schedule, paid)
    tot = total(counts)
    what = "%s with N = %d, dt = %r: pays %r, branches %r" % (name, N, dt, paid, counts)
    if name == "canon":
        assert len(paid) >= 3 and all(c.nonpos <= 1 and c.interior >= len(vec_s) // 2 for c in counts.values()), what
        # (node 0 at s = 0; with N = 10 the date 0.6 is dropped: the index reaches it on step 6, and 6 * 0.1 > 0.6)
    elif name == "before_dt":
        assert dates[0] < dt and 0 not in paid.values() and 1 in paid.values(), what
    elif name == "step1":
        assert paid.get(1) == 0, what
    elif name == "lastN":
        assert N in paid, what
    elif name == "beyondT":
        assert sorted(paid.values()) == [0] and max(dates) >= (N + 1) * dt, what
    elif name == "same_step":
        assert 0 in paid.values() and 1 not in paid.values() and int(dates[0] / dt) == int(dates[1] / dt), what
    elif name == "cluster":
        assert paid == {1: 0} and dt <= dates[4] < N * dt, what  # the fifth date lies inside the sweep and is not paid
    elif name == "unsorted":
        assert sorted(paid.values()) == [0, 2] and dt <= dates[1] < N * dt, what
    elif name == "big_cash":
        assert paid and all(c.nonpos >= 2 and c.interior >= 2 for c in counts.values()), what
    elif name in ("huge_cash", "pct_one"):
        assert paid and all(c.nonpos == len(vec_s) for c in counts.values()), what
    elif name == "pct_only":
        assert paid and tot.interior > 0 and all(a == 0.0 for a in schedule[1]), what
    elif name == "zero":
        assert paid and all(c.fallback >= 1 and c.nonpos <= 1 for c in counts.values()), what
    elif name == "negative":
        assert paid and all(c.fallback - c.below_s0 >= 1 for c in counts.values()), what
    elif name in ("every_step", "on_grid"):
        assert len(dates) == N and paid == {1: 0}, what  # one date per step, and the rule pays only the first
    elif name in ("alternate", "on_grid_odd"):
        assert sorted(paid) == list(range(1, N + 1, 2)), what
    elif name == "empty":
        assert not dates and not paid, what
    else:
        raise KeyError(name)
    return paid, counts
