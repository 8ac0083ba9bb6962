"""Rate and model-parameter regimes shared by the CPU and GPU regime tests (test_oracle_regimes.py, test_emu_regimes.py,
test_gpu_regimes.py), the rotation that puts several model regimes into one batch, and the power-of-two spot scaling.

The rest of the suite runs r_d = 0.025 throughout, r_f in {0, 0.007, 0.01, 0.02, 0.03, 0.04}, and model parameters from a
narrow box.  These values select code paths (hadi_core.h: q = r_d - r_f, half_rd, bc_rate = put ? -r_d : r_f, hr0; the strips'
A0 weights divided by -theta dt q; the team kernel's unit_e branch at bc_rate == 0; rho = 0 empties A0; a large kappa (eta - v)
makes the v-direction convection-dominated for the un-pivoted pentadiagonal LU)."""
import numpy as np

import common as Cm

CANONICAL_MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
CANONICAL_RATES = (Cm.R_D, Cm.R_F)

#         id     r_d      r_f                       what it reaches
RATES = [("R0",  0.0,     0.0),                   # q = 0, half_rd = 0, put bc_rate = 0 (the team kernel's unit_e with put data); no strips
         ("R1",  0.0,     0.02),                  # r_d = 0 with q < 0; put b2 == 0
         ("R2", -0.005,   0.0),                   # negative domestic rate: the put's edge value K e^{-r_d t} grows
         ("R3", -0.005,  -0.01),                  # both negative, q > 0
         ("R4",  0.01,    0.04),                  # q < 0
         ("R5",  0.08,    0.0),                   # large reaction term
         ("R6",  0.025,   0.025 * (1 + 1e-12)),   # q ~ -2.5e-14: strips stay ON with weights scaled by 1 / (theta dt q)
         ("R7",  0.03,    0.03)]                  # q = 0 with non-zero rates; no strips
RATE = {r[0]: r[1:] for r in RATES}
Q_ZERO = ("R0", "R7")
MODEL_RATES = (0.025, 0.01)  # (r_d, r_f) of the model regimes

#          id    rho     sigma  kappa  eta
MODELS = [("M0",) + CANONICAL_MODEL,
          ("M1",  0.0,    0.3,   1.5,   0.04),    # A0 == 0
          ("M2",  0.95,   0.3,   1.5,   0.04),
          ("M3", -0.999,  0.3,   1.5,   0.04),
          ("M4", -0.7,    1.5,   0.5,   0.04),    # Feller far off
          ("M5", -0.7,    0.05,  1.5,   0.04),    # nearly deterministic variance
          ("M6", -0.5,    0.3,   0.0,   0.04),    # no mean reversion
          ("M7", -0.5,    0.5,   10.0,  0.5),     # convection-dominated v-direction
          ("M8", -0.5,    0.9,   3.0,   0.3)]     # the existing upwind case
MODEL = {m[0]: m[1:] for m in MODELS}
SCALE_POWERS = (9, -7, 30, -30)


def rotating_models(n, c=0):
    """Instance k of a batch takes model (k + c) % 9: neighbours never share a model; [n] tuples (rho, sigma, kappa, eta)."""
    return [MODELS[(k + c) % len(MODELS)][1:] for k in range(n)]


def per_instance(models):
    """The rho_i .. eta_i of the C ABI for a list of models."""
    a = np.asarray(models, dtype=np.float64)
    return {"rho_i": a[:, 0].copy(), "sigma_i": a[:, 1].copy(), "kappa_i": a[:, 2].copy(), "eta_i": a[:, 3].copy()}


def scaled(k, vec_s, delta_s, U0, strikes=None, divs=None):
    """Spot axis, payoff, strikes and dividend AMOUNTS times 2^k (exact in fp64); the percentages and dates stay."""
    f = 2.0 ** k
    ks = None if strikes is None else [K * f for K in strikes]
    dd = None if divs is None else (list(divs[0]), [a * f for a in divs[1]], list(divs[2]))
    return vec_s * f, delta_s * f, U0 * f, ks, dd
