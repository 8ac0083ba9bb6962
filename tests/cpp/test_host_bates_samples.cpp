// C++ test of hadi_host::bates_sample_ladder, compute_base_prices_bates_samples and compute_jacobian_bates_samples
// (include/hadi_host.hpp).  Two 50x25 instances of calls (r_f = 0), 8 steps, snapshots after 2, 5 and 8 steps, three samples each (the
// node of S_0, two off-node spots with scales), per-instance jump laws: each mirror function once.  Prints every number as a
// hexadecimal double: tests/test_cpp_bates_samples.py makes the same calls through the Python mirror and compares bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "hadi_host.hpp"

using namespace hadi_host;

static void print(const char *tag, const std::vector<double> &v) {
    std::printf("%s 0", tag);
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}

int main() {
    const double S_0 = 100.0, V_0 = 0.04, T = 1.0, r_d = 0.025, r_f = 0.0, rho = -0.9, sigma = 0.3, kappa = 1.5, eta = 0.04;
    const double theta = 0.8, eps = 1e-6;
    const int m1 = 50, m2 = 25, n = 2, N = 8, total_size = (m1 + 1) * (m2 + 1);
    const double delta_t = T / N;
    Handle h(0);
    GridViews grids;
    buildMultipleGridViews(grids, n, m1, m2);
    DO_Workspace ws(n, total_size);
    for (int i = 0; i < n; ++i) {
        const double K = 100.0 + 5.0 * i;
        Grid g(m1, 8 * K, S_0, K, K / 5, m2, 5.0, V_0, 5.0 / 500);
        grids.set(i, g);
        for (int j = 0; j <= m2; j++)
            for (int k = 0; k <= m1; k++) ws.U[(size_t)i * total_size + k + j * (m1 + 1)] = std::max(g.Vec_s[k] - K, 0.0);
    }
    const std::vector<double> U_0 = ws.U;
    Samples smp;
    smp.spots = {S_0, 90.0, 110.5};
    smp.scales = {1.0, 1.1, 0.9};
    const std::vector<int> snaps = {2, 5, 8};
    Jumps law;
    law.lambda_i = {0.5, 2.0};
    law.mu_i = {-0.10, -0.05};
    law.sigma_i = {0.15, 0.10};
    int fails = 0;
    std::vector<double> lad, base, J8, b8, J5, b5;
    bates_sample_ladder(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, smp, snaps, law, lad);
    compute_base_prices_bates_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, smp,
                                      snaps, law, base);
    compute_jacobian_bates_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0, smp,
                                   snaps, law, true, J8, b8, eps);
    compute_jacobian_bates_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0, smp,
                                   snaps, law, false, J5, b5, eps);
    const size_t cells = (size_t)n * snaps.size() * 3;
    if (lad.size() != cells || base.size() != cells || J8.size() != cells * 8 || b8.size() != cells || J5.size() != cells * 5 || b5.size() != cells) {
        std::printf("FAIL sizes\n");
        fails++;
    }
    if (ws.U != U_0) { std::printf("FAIL the workspace was written\n"); fails++; }
    for (size_t e = 0; e < cells && !fails; e++) {
        if (!(lad[e] > 0.0) || std::fabs(b8[e] - base[e]) > 1e-10 * std::max(1.0, std::fabs(base[e]))) { std::printf("FAIL cell %zu\n", e); fails++; }
        for (int c = 5; c < 8; c++)
            if (!(std::fabs(J8[e * 8 + c]) > 1e-5)) { std::printf("FAIL jump column %d of cell %zu vanishes\n", c, e); fails++; }
    }
    {  // a NULL-sized jump array is the mirror's own error; (lambda + eps) delta_t > 1 the library's
        Jumps edge;
        edge.lambda = 1.0 / delta_t; edge.mu = -0.1; edge.sigma = 0.15;
        bool threw = false;
        std::vector<double> Jx, bx;
        try {
            compute_jacobian_bates_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                                           smp, snaps, edge, true, Jx, bx, eps);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL (lambda + eps) delta_t > 1 was accepted\n"); fails++; }
    }
    print("LADDER", lad);
    print("BASE", base);
    print("JAC8", J8);
    print("BASE8", b8);
    print("JAC5", J5);
    print("BASE5", b5);
    std::printf(fails ? "FAILED (%d)\n" : "all C++ Bates surface checks passed\n", fails);
    return fails ? 1 : 0;
}
