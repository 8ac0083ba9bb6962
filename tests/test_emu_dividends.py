"""CPU-only: the host routine that dates the dividends (hadi_plan.h, hadi_dividend_steps) against the plain-Python rule of
tests/dividend_schedules.py, and every named schedule of that module through each jump implementation the wave emulator
reaches (hadi_dividend_kernel in its layouts, hadi_small_kernel, hadi_small_seq_kernel, hadi_small_seq2_kernel,
hadi_team_kernel) against the oracle, which restates the reference's dating loop and linear scan on its own.  What the
emulator does not run -- the time loop of hadi_api.hip and the GPU build -- is tests/test_gpu_dividends.py."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import dividend_schedules as D
from test_emu_kernel_logic import _run, emu  # noqa: F401  (emu: the module-scoped fixture that builds the emulator library)


def _steps(emu, N, dt, dates, length):
    d = np.array(dates, dtype=np.float64)
    f = (C.c_int * length)(*([7] * length))
    emu.emu_dividend_steps.restype = None
    emu.emu_dividend_steps(N, C.c_double(dt), len(dates), d.ctypes.data_as(C.POINTER(C.c_double)), f, length)
    return list(f)


def test_dating_of_the_named_schedules(emu):
    vs = Cm.oracle_grids(50, 25, [100.0])[0][0]
    for N, T in ((9, 1.0), (10, 1.0), (20, 1.0), (3, 1.0), (30, 0.7), (8, 2.0)):
        dt = T / N
        for name, sch in D.named(N, dt, T).items():
            assert _steps(emu, N, dt, sch[0], N) == D.flags(N, dt, sch[0]), (name, N, T)
            assert _steps(emu, N, dt, sch[0], N + 5) == D.flags(N, dt, sch[0], N + 5), (name, N, T)
            if N >= 9:  # every named schedule reaches its branch from 9 steps on (the sequential passes' N = 3: four of them)
                D.requirement(name, N, dt, sch, vs)
            elif name in ("step1", "big_cash", "same_step", "zero"):
                D.requirement(name, N, dt, sch, vs)


def test_dating_of_twelve_steps_of_0_05(emu):
    """12 * 0.05 = 0.6000000000000001 > 0.6: the dividend dated 0.6 belongs to step 11 (0.55 <= 0.6 < 0.6000000000000001), and
    a date given as that product belongs to step 12."""
    assert 12 * 0.05 > 0.6
    assert D.paying_steps(20, 0.05, [0.6]) == {11: 0} and _steps(emu, 20, 0.05, [0.6], 20) == D.flags(20, 0.05, [0.6])
    assert D.paying_steps(20, 0.05, [12 * 0.05]) == {12: 0} and _steps(emu, 20, 0.05, [12 * 0.05], 20) == D.flags(20, 0.05, [12 * 0.05])
    assert _steps(emu, 20, 0.05, Cm.DIVS[0], 20) == D.flags(20, 0.05, Cm.DIVS[0])
    assert D.paying_steps(20, 0.05, Cm.DIVS[0]) == {4: 0, 8: 1, 11: 2, 16: 3}


def test_dating_of_random_schedules(emu):
    rng = random.Random(20240611)
    count, paid_total, multi, adjacent = 0, 0, 0, 0
    for _ in range(2400):
        N = rng.randint(1, 60)
        T = rng.choice([0.25, 0.7, 1.0, 1.5, 3.0, 0.1 * N, 0.05 * N])
        dt = T / N
        dates = D.random_schedule(rng, N, dt)[0]
        length = N + rng.choice([0, 0, 1, 7])
        want = D.flags(N, dt, dates, length)
        assert _steps(emu, N, dt, dates, length) == want, (N, T, dates)
        assert all(f == -1 for f in want[N:])
        steps = sorted(D.paying_steps(N, dt, dates))
        paid_total += len(steps)
        multi += len(steps) >= 2
        adjacent += any(b == a + 1 for a, b in zip(steps, steps[1:]))
        count += 1
    assert count >= 2000 and paid_total > count and multi > 200  # the campaign is not vacuous
    assert adjacent == 0  # (the rule never pays on two adjacent steps: see dividend_schedules.py)


# ---- every named schedule through every jump implementation of the emulator -------------------------------------------------
N_EMU = 9  # dt = 1/9 is not a binary fraction; unsorted needs 8 steps
PATHS = {
    # id: (m1, m2, strikes, variant, target_waves, kwargs of _run)
    "stream_40x12_DIV": (40, 12, [100.0], O.DIV, 8, dict(r_f=0.01)),
    "stream_40x12_AM_DIV_pair": (40, 12, [100.0], O.AM_DIV, 8, dict(r_f=0.01)),
    "stream_40x12_AM_DIV_P": (40, 12, [100.0], O.AM_DIV, 8, dict(r_f=0.01, scheme=3)),
    "stream_40x12_AM_DIV_put": (40, 12, [100.0], O.AM_DIV, 8, dict(put=True)),
    "stream_72x70_DIV": (72, 70, [100.0], O.DIV, 3, dict()),                      # two nodes per lane, chunked column pass
    "stream_600x16_DIV": (600, 16, [100.0], O.DIV, 8, dict(r_f=0.01)),            # two wavefronts per row
    "small4_50x25_AM_DIV": (50, 25, [100.0], O.AM_DIV, 8, dict(small=1, put=True)),
    "small8_50x25_DIV": (50, 25, [100.0], O.DIV, 8, dict(small=2, r_f=0.01)),
    "seq_50x25_DIV": (50, 25, [100.0], O.DIV, 8, dict(small=3, r_f=0.01)),
    "seq2_50x25_DIV_odd_batch": (50, 25, [105.0, 95.0, 100.0], O.DIV, 8, dict(small=5, r_f=0.01, put=True)),
    "team4_150x20_DIV": (150, 20, [100.0], O.DIV, 8, dict(small=4, r_f=0.01)),
    "team8_300x20_DIV_put": (300, 20, [100.0], O.DIV, 8, dict(small=4, r_f=0.01, put=True)),
}


@pytest.mark.parametrize("name", D.NAMES)
@pytest.mark.parametrize("path", list(PATHS))
def test_named_schedules_through_every_jump_of_the_emulator(emu, path, name):
    m1, m2, strikes, variant, tw, kw = PATHS[path]
    dt = Cm.T / N_EMU
    sch = D.named(N_EMU, dt, Cm.T)[name]
    vs = Cm.oracle_grids(m1, m2, strikes)[0]
    for k in range(len(strikes)):
        D.requirement(name, N_EMU, dt, sch, vs[k])
    _run(emu, m1, m2, N_EMU, strikes, variant, tw, divs=sch, **kw)
