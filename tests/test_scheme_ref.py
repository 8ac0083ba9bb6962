"""tests/scheme_ref.py (the test-side restatement of Douglas, Craig-Sneyd, Modified Craig-Sneyd and Hundsdorfer-Verwer that the
GPU tests of the MCS / HV kernels compare against) checked on the CPU: its Douglas and Craig-Sneyd are the oracle's, bit for bit,
and MCS at theta = 1/2 is Craig-Sneyd exactly."""
import numpy as np
import pytest

from oracle import oracle as O

import common as Cm
import scheme_ref as S

SHAPES = [(40, 20, 12, 0.007), (64, 33, 7, 0.007), (30, 16, 5, 0.0)]


def _case(m1, m2, N, r_f, n=2):
    strikes = Cm.strikes_for(n)
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, strikes)
    p = Cm.oracle_params(m1, m2, N, "EU", r_f=r_f)
    return p, (vs, vv, ds, dv), U0


@pytest.mark.parametrize("m1,m2,N,r_f", SHAPES)
@pytest.mark.parametrize("scheme", [S.DOUGLAS, S.CS])
def test_restatement_equals_the_oracle_bit_for_bit(m1, m2, N, r_f, scheme):
    p, g, U0 = _case(m1, m2, N, r_f)
    U = S.solve_batch(p, *g, U0, scheme)
    p.scheme = scheme
    Uo, _, _ = O.solve_batch(p, *g, U0)
    assert np.array_equal(U, Uo), np.abs(U - Uo).max()


@pytest.mark.parametrize("m1,m2,N,r_f", SHAPES)
def test_mcs_at_one_half_is_craig_sneyd(m1, m2, N, r_f):
    p, g, U0 = _case(m1, m2, N, r_f)
    assert np.array_equal(S.solve_batch(p, *g, U0, S.MCS, 0.5), S.solve_batch(p, *g, U0, S.CS, 0.5))


def test_mcs_and_hv_beat_douglas_at_twenty_steps():
    """The reason for the two schemes (in 't Hout & Foulon): at the step counts of calibration (N = 20) their time error is far
    below Douglas's, which is first order with the mixed-derivative term.  Reference: HV at N = 640 on the same space grid."""
    m1, m2 = 50, 25
    vs, vv, ds, dv, U0 = Cm.oracle_grids(m1, m2, [100.0])
    g = (vs, vv, ds, dv)

    def err(N, scheme, theta):
        p = Cm.oracle_params(m1, m2, N, "EU", r_f=0.007)
        return S.solve_batch(p, *g, U0, scheme, theta)[0]

    ref = err(640, S.HV, 0.5 + 3 ** 0.5 / 6)
    e = {sc: S.time_error(err(20, sc, th), ref, vs[0], vv[0], m1, m2)
         for sc, th in ((S.DOUGLAS, 0.5), (S.MCS, 1.0 / 3.0), (S.HV, 0.5 + 3 ** 0.5 / 6))}
    assert e[S.MCS] <= e[S.DOUGLAS] / 20 and e[S.HV] <= e[S.DOUGLAS] / 8, e
