"""CPU-only check, under the wave emulator, of what the resident sweep (hadi_sweep_resident, csrc/hadi_k_resident.h) does at its
phase boundaries from the second step on: the s-coefficient arrays and RT are staged by a block's first step alone, the column
phase requests its chunk table -- and, where every wavefront owns the same v-rows in both phases (strips of 33 rows, the
"fast path": 256 < m1 <= 512 with m2 in 256 .. 263), its first two tiles -- before the block meets, and the short column tile runs
second.  Every case runs at least three steps, so steps after the first are exercised, and is compared against the oracle (1e-10)
and against the emulator's streaming path at the same strip geometry (1e-13; `_check` of test_emu_resident.py asserts both).
Well-conditioned grids only, asserted (the 30x rule of DESIGN.md section 2): the 1e-10 bound belongs to such grids."""
import pytest

import common as Cm
from test_emu_resident import PER_INSTANCE_PAR, _check, _solve, _strip_rows, emu  # noqa: F401  (emu: the module's fixture)

N_STEPS = 3


def _fast_path(m2):
    """Strips of HADI_LC = 33 rows: strip w and column chunk w are the same rows."""
    return _strip_rows(m2)[0] == 33


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("m2", [231, 256, 263])
@pytest.mark.parametrize("m1", [257, 512])
def test_eight_chunk_shapes(emu, m1, m2, n):
    """Both ends of the row width with eight column chunks: m2 = 256 (the benchmarked grid, a last strip of 26 rows) and 263
    (eight full strips) are on the fast path; m2 = 231 has eight chunks too but strips of 29 rows, so it must stay off it."""
    assert _fast_path(m2) == (m2 >= 256)
    strikes = Cm.well_conditioned_strikes(m1, n)
    vs, vv, ds, dv, U0, Ur, Us, P = _solve(emu, m1, m2, N_STEPS, strikes, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    assert P == (m2 + 33) // 33
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [N_STEPS] * n, [Cm.T / N_STEPS] * n)


@pytest.mark.parametrize("m1,m2,P", [(300, 80, 3), (400, 150, 5)])
def test_shapes_off_the_fast_path(emu, m1, m2, P):
    """Strips of 11 and 19 rows against chunks of 33: the tile loads stay behind the block's meeting; 3 and 5 chunks leave
    idle column wavefronts, which must keep the barrier count of the others from the second step on as well."""
    assert not _fast_path(m2)
    strikes = Cm.well_conditioned_strikes(m1, 2)
    vs, vv, ds, dv, U0, Ur, Us, p_chunks = _solve(emu, m1, m2, N_STEPS, strikes, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    assert p_chunks == P
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, [N_STEPS] * 2, [Cm.T / N_STEPS] * 2)


def test_fast_path_per_instance_maturities(emu):
    """One block stops after its first step -- it never runs a step on staged data -- one runs three, one two."""
    m1, m2 = 512, 256
    assert _fast_path(m2)
    Ns, Ts = [1, 3, 2], [0.2, 0.9, 0.5]
    dts = [t / s for t, s in zip(Ts, Ns)]
    strikes = Cm.well_conditioned_strikes(m1, 3)
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, 1, strikes, Ns, dts, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts)


def test_fast_path_per_instance_parameters_and_put_data(emu):
    """Three instances with their own (rho, sigma, kappa, eta) and strike, put payoff and put boundary data, three steps: RT,
    the coefficient arrays or the instance scalars taken from another instance, or left stale, show against the oracle."""
    m1, m2 = 257, 256
    assert _fast_path(m2)
    strikes = Cm.well_conditioned_strikes(m1, 3)
    Ns, dts = [N_STEPS] * 3, [Cm.T / N_STEPS] * 3
    vs, vv, ds, dv, U0, Ur, Us, _ = _solve(emu, m1, m2, 1, strikes, Ns, dts, par=PER_INSTANCE_PAR, put=True, V0=Cm.v0_for(m2))
    Cm.assert_well_conditioned(ds, dv)
    _check(m1, m2, vs, vv, ds, dv, U0, Ur, Us, Ns, dts, par=PER_INSTANCE_PAR, put=True, strikes=strikes)
