"""The LM normal equations for 1 .. 8 parameters on the host (hadi_lm_partials_n, hadi_lm_solve_n) and their Python wrappers, which
take the width from J.shape[1] and from the partials' length: against numpy, bit-equal to the five-parameter functions at width 5,
and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H
from pde_based_heston_solver_gpu_accelerated_amd import _native as nat

_dp = nat._dp
INVALID = 1


def ptr(a):
    return a.ctypes.data_as(_dp)


def random_rows(n, w, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal((n, w)) * rng.uniform(0.1, 10.0, w)), rng.standard_normal(n)


def numpy_partials(J, r):
    return np.concatenate([(J.T @ J).reshape(-1), J.T @ r, [r @ r]])


@pytest.mark.parametrize("w", [1, 5, 8])
@pytest.mark.parametrize("n", [1, 37, 500])
def test_partials_against_numpy(w, n):
    J, r = random_rows(n, w, 100 * w + n)
    part = H.lm_partials(J, r)
    want = numpy_partials(J, r)
    assert part.shape == (w * w + w + 1,)
    # every sum is n products added one by one: n ulp of the sum of the magnitudes
    bound = n * np.finfo(float).eps * numpy_partials(np.abs(J), np.abs(r))
    assert (np.abs(part - want) <= bound).all()
    assert np.array_equal(part[:w * w].reshape(w, w), part[:w * w].reshape(w, w).T)
    raw = np.full(w * w + w + 1, np.nan)
    assert nat.lib().hadi_lm_partials_n(n, w, ptr(J), ptr(r), ptr(raw)) == 0
    assert np.array_equal(raw, part)


def test_width_5_is_the_five_parameter_functions_bit_for_bit():
    lib = nat.lib()
    for n, seed in ((1, 1), (12, 2), (333, 3)):
        J, r = random_rows(n, 5, seed)
        a, b = np.empty(31), np.empty(31)
        assert lib.hadi_lm_partials(n, ptr(J), ptr(r), ptr(a)) == 0 and lib.hadi_lm_partials_n(n, 5, ptr(J), ptr(r), ptr(b)) == 0
        assert np.array_equal(a, b) and np.array_equal(a, H.lm_partials(J, r))
        for lam in (0.0, 0.01, 10.0):
            da, db = np.empty(5), np.empty(5)
            if n >= 5 or lam > 0.0:
                assert lib.hadi_lm_solve(ptr(a), lam, ptr(da)) == 0 and lib.hadi_lm_solve_n(5, ptr(a), lam, ptr(db)) == 0
                assert np.array_equal(da, db) and np.array_equal(da, H.lm_solve(a, lam))
        du = np.empty(5)
        assert lib.hadi_compute_parameter_update(n, ptr(J), ptr(r), 0.01, ptr(du)) == 0
        assert np.array_equal(du, H.lm_solve(a, 0.01)) and np.array_equal(du, H.compute_parameter_update(J, r, 0.01))


@pytest.mark.parametrize("w", [1, 5, 8])
def test_solve_against_numpy_on_a_well_conditioned_system(w):
    """J^T J = Q diag(1 .. 3) Q^T + the LM damping: condition below 4, so 1e-12 relative leaves four digits over the elimination's
    w^2 cond eps."""
    rng = np.random.default_rng(7 + w)
    Q, _ = np.linalg.qr(rng.standard_normal((w, w)))
    A = Q @ np.diag(np.linspace(1.0, 3.0, w)) @ Q.T
    A = 0.5 * (A + A.T)
    g = rng.standard_normal(w)
    part = np.concatenate([A.reshape(-1), g, [1.0]])
    for lam in (0.0, 0.01, 1.0):
        want = np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
        got = H.lm_solve(part, lam)
        assert got.shape == (w,)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_solve_pivots():
    """A zero on the diagonal where the column below is not zero: the elimination swaps rows."""
    A = np.array([[0.0, 2.0, 0.0], [2.0, 1.0, 0.5], [0.0, 0.5, 3.0]])
    g = np.array([1.0, -2.0, 0.5])
    got = H.lm_solve(np.concatenate([A.reshape(-1), g, [0.0]]), 0.0)
    assert np.abs(got - np.linalg.solve(A, g)).max() <= 1e-14


def test_refusals():
    lib = nat.lib()
    J, r = random_rows(4, 8, 5)
    out, d = np.zeros(73), np.zeros(8)
    for bad in (0, -1, 9, 100):
        assert lib.hadi_lm_partials_n(4, bad, ptr(J), ptr(r), ptr(out)) == INVALID
        assert lib.hadi_lm_solve_n(bad, ptr(out), 0.01, ptr(d)) == INVALID
    assert lib.hadi_lm_partials_n(-1, 8, ptr(J), ptr(r), ptr(out)) == INVALID
    assert lib.hadi_lm_partials_n(4, 8, None, ptr(r), ptr(out)) == INVALID
    assert lib.hadi_lm_partials_n(4, 8, ptr(J), ptr(r), None) == INVALID
    assert lib.hadi_lm_solve_n(8, None, 0.01, ptr(d)) == INVALID and lib.hadi_lm_solve_n(8, ptr(out), 0.01, None) == INVALID
    assert lib.hadi_lm_partials_n(0, 8, None, None, ptr(out)) == 0 and not out.any()  # (no rows: zeros)
    with pytest.raises(ValueError):
        H.lm_partials(np.zeros((3, 9)), np.zeros(3))
    with pytest.raises(ValueError):
        H.lm_solve(np.zeros(32), 0.01)
    assert lib.hadi_version() == 2
