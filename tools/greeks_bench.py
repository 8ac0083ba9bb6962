#!/usr/bin/env python3
"""Wall time of three ways to the Greeks of a batch, on one GPU, device-resident inputs, alternating order on one box:
   node    HestonADI.compute_greeks, node row only            ([n][8] leaves the device)
   ladder  HestonADI.compute_greeks with the spot ladder      ([n][m1+1][8] as well)
   field   DO_timestepping, then U (and lambda_bar) to the host and the ladder's price, delta, gamma, dv, dvv, dsv and lambda
           columns restated there in numpy (theta is left out: it would need the operators on the host as well)
for  C3   512 American puts with discrete dividends, 256x128, 500 steps
     C2   256 European calls, 512x256, 1000 steps.
The strikes are the bench ladder 85 + 30 k / (n - 1); part of their s-grids break the 30x rule of DESIGN.md section 2, which is
harmless for a timing -- the "device ladder vs host restatement" line is a plausibility check of the two paths on the same
field, carrying those grids' conditioning in gamma, not a stencil test (tests/test_gpu_greeks.py is).
Each timing is a host clock around work that ends in a device synchronise.  `python tools/greeks_bench.py > profiles/<tag>.txt`."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import pde_based_heston_solver_gpu_accelerated_amd as H

S_0, V_0, T, r_d, r_f = 100.0, 0.04, 1.0, 0.025, 0.007
rho, sigma, kappa, eta, theta = -0.9, 0.3, 1.5, 0.04, 0.8
dev = torch.device("cuda:0")
solver = H.HestonADI(0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def w3(x, k):
    """Three-point first / second derivative weights at the interior nodes k of the axis x: ([3][len k], [3][len k])."""
    a, b = x[k] - x[k - 1], x[k + 1] - x[k]
    return (np.stack([-b / (a * (a + b)), (b - a) / (a * b), a / (b * (a + b))]),
            np.stack([2 / (a * (a + b)), -2 / (a * b), 2 / (b * (a + b))]))


def host_ladder(g, U, lam, m1, m2):
    """Interior nodes of the row of V_0, every instance: price, delta, gamma, dv, dvv, dsv, lambda; [n][m1-1][7]."""
    n = U.shape[0]
    out = np.empty((n, m1 - 1, 7))
    ii = np.arange(1, m1)
    for k in range(n):
        vv, vs = g.Vec_v[k], g.Vec_s[k]
        j0 = int(np.nonzero(np.abs(vv - V_0) < 1e-10)[0][0])
        F = U[k].reshape(m2 + 1, m1 + 1)
        (s1, s2), (v1, v2) = w3(vs, ii), w3(vv, np.array([j0]))
        rows = F[j0 - 1:j0 + 2]
        d = s1[0] * rows[:, :-2] + s1[1] * rows[:, 1:-1] + s1[2] * rows[:, 2:]
        out[k, :, 0] = rows[1, 1:-1]
        out[k, :, 1] = d[1]
        out[k, :, 2] = s2[0] * rows[1, :-2] + s2[1] * rows[1, 1:-1] + s2[2] * rows[1, 2:]
        out[k, :, 3] = v1[0] * rows[0, 1:-1] + v1[1] * rows[1, 1:-1] + v1[2] * rows[2, 1:-1]
        out[k, :, 4] = v2[0] * rows[0, 1:-1] + v2[1] * rows[1, 1:-1] + v2[2] * rows[2, 1:-1]
        out[k, :, 5] = v1[0] * d[0] + v1[1] * d[1] + v1[2] * d[2]
        out[k, :, 6] = 0.0 if lam is None else lam[k].reshape(m2 + 1, m1 + 1)[j0, 1:-1]
    return out


def config(name, m1, m2, N, n, variant, put):
    ks = [100.0] if n == 1 else [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    g = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, ks)
    U0h = g.put_payoff(ks) if put else g.call_payoff(ks)
    gd, U0 = g.to(dev), torch.from_numpy(U0h).to(dev)
    U, lam = torch.empty_like(U0), (torch.zeros_like(U0) if variant in (H.AM, H.AM_DIV) else None)
    div = H.Dividends([0.2, 0.4, 0.6, 0.8], [0.5, 0.3, 0.2, 0.1], [0.02] * 4) if variant in (H.DIV, H.AM_DIV) else None
    kw = dict(variant=variant, dividends=div, option_type=H.PUT if put else H.CALL, strikes=ks if put else None)
    args = (m1, m2, N, T / N, theta, r_d, r_f, rho, sigma, kappa, eta, gd)
    res = {}

    def node():
        res["node"] = solver.compute_greeks(*args, U0, S_0, V_0, **kw).cpu().numpy()

    def ladder():
        a, b = solver.compute_greeks(*args, U0, S_0, V_0, ladder=True, **kw)
        res["ladder"] = b.cpu().numpy()

    def field():
        U.copy_(U0)
        solver.DO_timestepping(*args, U, U_0=U0 if lam is not None else None, lambda_bar=lam, **kw)
        res["field"] = host_ladder(g, U.cpu().numpy(), None if lam is None else lam.cpu().numpy(), m1, m2)

    ways = [("node", node), ("ladder", ladder), ("field", field)]
    for _, fn in ways:  # warm-up of every shape the timed window uses
        fn(); torch.cuda.synchronize()
    times = {k: [] for k, _ in ways}
    for r in range(ROUNDS):
        for k, fn in (ways if r % 2 == 0 else ways[::-1]):  # alternating order
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    sel = [0, 1, 2, 3, 4, 5, 7]
    same = np.abs(res["ladder"][:, 1:-1, sel] - res["field"]).max(axis=(0, 1)) / np.abs(res["field"]).max(axis=(0, 1)).clip(1e-300)
    print("%s: %d x %dx%dx%d, %s; kernels: %s" % (name, n, m1, m2, N, "American puts with dividends" if put else "European calls",
                                                  solver.describe_last_sweep()))
    for k, _ in ways:
        t = np.array(times[k]) * 1e3
        print("  %-6s ms per call: %s  median %.2f" % (k, " ".join("%.2f" % x for x in t), np.median(t)))
    print("  bytes to the host: node %d, ladder %d, field %d" % (res["node"].nbytes, res["node"].nbytes + res["ladder"].nbytes,
                                                                 U0h.nbytes * (2 if lam is not None else 1)))
    print("  device ladder vs host restatement, max |diff| / max |column| (price delta gamma dv dvv dsv lambda): %s"
          % " ".join("%.1e" % x for x in same))


print("device: %s; %d alternating rounds per configuration" % (solver.device_info(), ROUNDS))
config("C3", 256, 128, 500, 512, H.AM_DIV, True)
config("C2", 512, 256, 1000, 256, H.EU, False)
