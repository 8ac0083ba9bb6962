"""The property the maturity ladder rests on, on the CPU oracle: the state after step n of an N-step solve IS the n-step solve,
bit for bit -- so "snapshot q of a ladder call" can be defined as "what the same call with N = snap_steps[q] returns"
(include/hadi.h).  Grid 50x25, N = 20, dt = T / 20, the canonical dividend schedule; n runs over every step, so each paying step
and the step after it are covered.

The property has one condition, pinned here too: the call's boundary vector carries exp(-r_f dt (N - 1))
(oracle/heston_oracle.c bc_initialize, the reference's hes_boundary_kernels.hpp:56), so it holds for calls with r_f = 0 (the
canonical rate) and for puts (time factor exp(-r_d dt n) only) and FAILS for calls with r_f != 0 -- which is why the library's
ladder entry points refuse those."""
import math

import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import scheme_ref as S

M1, M2, N = 50, 25, 20
DT = Cm.T / N
K = 100.0


@pytest.fixture(scope="module")
def grid():
    vs, vv, ds, dv, U0 = Cm.oracle_grids(M1, M2, [K])
    return vs[0], vv[0], ds[0], dv[0], U0[0]


def _params(n, variant, r_f=Cm.R_F, put=False):
    v = Cm.VARIANT[variant]
    return O.make_params(M1, M2, n, DT, Cm.THETA, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, v,
                         Cm.DIVS if v in (O.DIV, O.AM_DIV) else None, option_type=O.PUT if put else O.CALL,
                         strikes=K if put else None)


def _state_after(n, variant, g, U0, **kw):
    """U after step n of the N-step solve (the oracle's dump)."""
    vs, vv, ds, dv, _ = g
    return O.solve(_params(N, variant, **kw), vs, vv, ds, dv, U0, U0 if "AM" in variant else None, dump_step=n)[2]["Unext"]


def _solve(n, variant, g, U0, **kw):
    vs, vv, ds, dv, _ = g
    return O.solve(_params(n, variant, **kw), vs, vv, ds, dv, U0, U0 if "AM" in variant else None)[0]


def _paying_steps():
    """Steps at whose start a dividend is paid, by the dating rule of include/hadi.h."""
    out, idx = [], 0
    dates = Cm.DIVS[0]
    for n in range(1, N + 1):
        if idx < len(dates) and n * DT <= dates[idx] < (n + 1) * DT:
            out.append(n)
        if idx < len(dates) and n * DT > dates[idx]:
            idx += 1
    return out


def test_the_schedule_pays_inside_the_ladder():
    pay = _paying_steps()
    assert len(pay) >= 2 and all(1 <= n < N for n in pay)


@pytest.mark.parametrize("variant", ["EU", "AM", "DIV", "AM_DIV"])
def test_douglas_prefix_is_the_shorter_solve(grid, variant):
    U0 = grid[4]
    for n in range(1, N + 1):
        assert np.array_equal(_state_after(n, variant, grid, U0), _solve(n, variant, grid, U0)), (variant, n)


def test_dividend_steps_change_the_state(grid):
    """(so the comparison above would notice a paying step dated differently in the two solves)"""
    U0 = grid[4]
    for n in _paying_steps():
        assert not np.array_equal(_solve(n, "DIV", grid, U0), _solve(n, "EU", grid, U0)), n


def _scheme_states(p, g, U0, scheme):
    """tests/scheme_ref.py's step, restated so that every intermediate state is visible (pinned to solve_one below)."""
    vs, vv, ds, dv, _ = g
    op = S._Ops(p, vs, vv, ds, dv, U0)
    b, b0, b1, b2 = op.b, op.b0, op.b1, op.b2
    dt, r_f, th = p.delta_t, p.r_f, p.theta
    U = np.array(U0, dtype=np.float64)
    for n in range(1, p.N + 1):
        A0U, A1U, A2U = op.A(0, U), op.A(1, U), op.A(2, U)
        e_n, e_nm1 = math.exp(r_f * dt * n), math.exp(r_f * dt * (n - 1))
        Y0 = U + dt * (A0U + A1U + A2U + b * e_nm1)
        Y1 = op.solve(1, Y0 + th * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
        Y2 = op.solve(2, Y1 + th * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
        A0Y2, A1Y2, A2Y2 = op.A(0, Y2), op.A(1, Y2), op.A(2, Y2)
        d0 = (A0Y2 + b0 * e_n) - (A0U + b0 * e_nm1)
        d = (A0Y2 + A1Y2 + A2Y2 + b * e_n) - (A0U + A1U + A2U + b * e_nm1)
        if scheme == S.MCS:
            Yh = Y0 + th * dt * d0 + (0.5 - th) * dt * d
            Yt = op.solve(1, Yh + th * dt * (b1 * e_n - (A1U + b1 * e_nm1)))
            U = op.solve(2, Yt + th * dt * (b2 * e_n - (A2U + b2 * e_nm1)))
        else:
            Yh = Y0 + 0.5 * dt * d
            Yt = op.solve(1, Yh - th * dt * A1Y2)
            U = op.solve(2, Yt - th * dt * A2Y2)
        yield n, U


@pytest.mark.parametrize("scheme,theta", [(S.MCS, 1.0 / 3.0), (S.HV, 0.5 + math.sqrt(3.0) / 6.0)], ids=["MCS", "HV"])
def test_scheme_prefix_is_the_shorter_solve(grid, scheme, theta):
    vs, vv, ds, dv, U0 = grid

    def params(n):
        return O.make_params(M1, M2, n, DT, theta, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)

    states = dict(_scheme_states(params(N), grid, U0, scheme))
    assert np.array_equal(states[N], S.solve_one(params(N), vs, vv, ds, dv, U0, scheme))  # the restated loop is scheme_ref's
    for n in range(1, N):
        assert np.array_equal(states[n], S.solve_one(params(n), vs, vv, ds, dv, U0, scheme)), n


def test_the_condition_call_data_need_a_zero_foreign_rate(grid):
    """Calls with r_f != 0: the boundary vector of the N-step solve differs from the n-step solve's, and so do the states.  Puts
    with the same rates keep the property."""
    vs, vv, ds, dv, U0 = grid
    r_f = 0.007
    for n in (1, 5, 19):
        assert not np.array_equal(_state_after(n, "EU", grid, U0, r_f=r_f), _solve(n, "EU", grid, U0, r_f=r_f)), n
    assert np.array_equal(_state_after(N, "EU", grid, U0, r_f=r_f), _solve(N, "EU", grid, U0, r_f=r_f))
    P0 = np.tile(np.maximum(K - vs, 0.0), M2 + 1)
    for n in (1, 5, 12, 13, 19, 20):
        for variant in ("EU", "AM", "DIV"):
            assert np.array_equal(_state_after(n, variant, grid, P0, r_f=r_f, put=True), _solve(n, variant, grid, P0, r_f=r_f, put=True)), (variant, n)
