"""The resident sweep's phase boundaries on the GPU (csrc/hadi_k_resident.h): coefficient arrays and RT staged by a block's first
step alone, the column phase's table and -- on the fast path, strips of 33 rows -- its first two tiles requested before the
block meets, the short column tile second.  Every case asserts from describe_last_sweep() that hadi_sweep_resident<8> ran,
compares with "resident_sweep" = 0 on the same handle (<= 1e-13 max|U|) and with the oracle (1e-10 max|U|) on grids that obey
the 30x conditioning rule (asserted by `_inputs`).  The oracle runs on every instance at 300x80 and on the fixed subset of
test_gpu_resident.py (the XCD remap's first round and the ends) at the larger grids, whose every instance is still compared
with the streaming path."""
import numpy as np
import pytest

import common as Cm
from test_gpu_resident import MODEL, RESIDENT, SUBSET, _inputs, _oracle_check, _resident_and_streaming, _run, strict_solver  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m1,m2,rs", [(257, 231, 29), (512, 256, 33), (512, 263, 33), (300, 80, 11)])
def test_four_steps(solver, m1, m2, rs):
    """256 instances, 4 steps: three of them run on what the first staged.  512x256 and 512x263 are on the fast path; 300x80
    (strips of 11 rows, five idle column wavefronts) and 257x231 (eight chunks, but strips of 29 rows) are off it."""
    n, N = 256, 4
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0, strip=1)
    assert "(strips of %d rows)" % rs in d, d
    _oracle_check(m1, m2, grids, U0, U, range(n) if m1 == 300 else SUBSET(n), N=N)


def test_per_instance_maturities_250_instances(solver):
    """250 instances of 512x256 (a padded grid of 256 blocks, six of them without an instance) with N_i = 1 .. 6: blocks that
    stop after the first step next to blocks that run five more on staged data."""
    m1, m2, n = 512, 256, 250
    Ns = [(1, 6, 2, 5, 3, 4)[k % 6] for k in range(n)]
    Ts = [0.25 + 0.1 * (k % 5) for k in range(n)]
    per = {"N_i": Ns, "delta_t_i": [t / s for t, s in zip(Ts, Ns)]}
    for key, v in zip(("rho_i", "sigma_i", "kappa_i", "eta_i"), MODEL):
        per[key] = [v] * n
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, 1, grids, U0, per=per)
    _oracle_check(m1, m2, grids, U0, U, SUBSET(n), per=per, threads=6)


def test_second_launch_restages(solver):
    """Two calls on one handle, the same geometry, other kappa and sigma: the second launch must stage its own coefficient
    arrays and RT (a launch that kept the first call's would differ from the streaming path and from the oracle)."""
    m1, m2, n, N = 512, 256, 256, 4
    _, grids, U0 = _inputs(m1, m2, n)
    fields = []
    for model in (MODEL, (MODEL[0], 0.55, 3.0, MODEL[3])):
        U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0, model=model)
        _oracle_check(m1, m2, grids, U0, U, SUBSET(n), N=N, model=model)
        fields.append(U)
    assert np.abs(fields[0] - fields[1]).max() > 1e-6 * np.abs(fields[0]).max()  # (the parameters matter)


def test_bit_identity_with_the_strict_build(solver, strict_solver):
    """512x256 x 256 x 4 steps against libhadi_strict.so (every counted vmcnt wait a full drain): bit for bit."""
    m1, m2, n, N = 512, 256, 256, 4
    _, grids, U0 = _inputs(m1, m2, n)
    U, d, _ = _resident_and_streaming(solver, m1, m2, N, grids, U0)
    Ux, dx = _run(strict_solver, m1, m2, N, grids, U0, 1)
    assert RESIDENT in dx and d == dx, (d, dx)
    assert np.array_equal(U, Ux)
    _oracle_check(m1, m2, grids, U0, U, SUBSET(n), N=N)
