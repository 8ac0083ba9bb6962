// C++ test of hadi_host::compute_jacobian_bates_jumps, lm_partials_n and lm_solve_n (include/hadi_host.hpp).
// One 50x25 batch of four puts with dividends, 20 steps: the eight-column Jacobian with per-instance jump laws (the third has
// intensity 0: its mu_J and sigma_J columns are exactly zero), then with one shared law, whose first five columns and base prices
// are set beside compute_jacobian_bates'; the 73 partial sums and one LM step from the second Jacobian.  Prints every number as a
// hexadecimal double: tests/test_cpp_jumps8.py makes the same calls through the Python mirror and compares bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "hadi_host.hpp"

using namespace hadi_host;

int main() {
    const double S_0 = 100.0, V_0 = 0.04, T = 1.0, r_d = 0.025, r_f = 0.007, rho = -0.9, sigma = 0.3, kappa = 1.5, eta = 0.04;
    const double theta = 0.8, eps = 1e-6;
    const int m1 = 50, m2 = 25, n = 4, N = 20, total_size = (m1 + 1) * (m2 + 1);
    const double delta_t = T / N;
    Handle h(0);
    PutStrikes strikes(n);
    for (int i = 0; i < n; ++i) strikes[i] = 90.0 + 5.0 * i;
    GridViews grids;
    buildMultipleGridViews(grids, n, m1, m2);
    std::vector<double> U_0((size_t)n * total_size);
    for (int i = 0; i < n; ++i) {
        const double K = strikes[i];
        Grid g(m1, 8 * K, S_0, K, K / 5, m2, 5.0, V_0, 5.0 / 500);
        grids.set(i, g);
        for (int j = 0; j <= m2; j++)
            for (int k = 0; k <= m1; k++) U_0[(size_t)i * total_size + k + j * (m1 + 1)] = std::max(K - g.Vec_s[k], 0.0);
    }
    Dividends div{{0.2, 0.4, 0.6, 0.8}, {0.5, 0.3, 0.2, 0.1}, {0.02, 0.02, 0.02, 0.02}};
    Jumps per;
    per.lambda_i = {0.5, 2.0, 0.0, 0.3};
    per.mu_i = {-0.10, -0.05, 0.0, 0.10};
    per.sigma_i = {0.15, 0.10, 0.2, 0.30};
    Jumps shared;
    shared.lambda = 0.5; shared.mu = -0.10; shared.sigma = 0.15;
    int fails = 0;
    std::vector<double> J8p, basep, J8, base8, J5, base5;
    compute_jacobian_bates_jumps(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                                 per, J8p, basep, eps, HADI_DIV, &div, &strikes);
    compute_jacobian_bates_jumps(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                                 shared, J8, base8, eps, HADI_DIV, &div, &strikes);
    compute_jacobian_bates(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                           shared, J5, base5, eps, HADI_DIV, &div, &strikes);
    if (J8p.size() != (size_t)n * 8 || J8.size() != (size_t)n * 8 || basep.size() != (size_t)n || base8.size() != (size_t)n) {
        std::printf("FAIL sizes\n");
        fails++;
    }
    if (J8p[2 * 8 + 6] != 0.0 || J8p[2 * 8 + 7] != 0.0 || J8p[2 * 8 + 5] == 0.0) { std::printf("FAIL the zero-intensity instance's jump columns\n"); fails++; }
    for (int i = 0; i < n; i++) {  // the launchers' bounds (the two calls may run different pass kernels: 24 instances against 36)
        if (std::fabs(base8[i] - base5[i]) > 1e-10 * std::max(1.0, std::fabs(base5[i]))) { std::printf("FAIL base %d\n", i); fails++; }
        for (int c = 0; c < 5; c++)
            if (std::fabs(J8[(size_t)i * 8 + c] - J5[(size_t)i * 5 + c]) > 2e-4) { std::printf("FAIL column %d of %d\n", c, i); fails++; }
        for (int c = 5; c < 8; c++)
            if (!(std::fabs(J8[(size_t)i * 8 + c]) > 1e-3)) { std::printf("FAIL jump column %d of %d vanishes\n", c, i); fails++; }
    }
    {  // (lambda + eps) delta_t > 1 is refused where lambda delta_t = 1 is a valid law
        Jumps edge = shared;
        edge.lambda = 1.0 / delta_t;
        bool threw = false;
        std::vector<double> Jx, bx;
        try {
            compute_jacobian_bates_jumps(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids,
                                         U_0, edge, Jx, bx, eps, HADI_DIV, &div, &strikes);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL (lambda + eps) delta_t > 1 was accepted\n"); fails++; }
    }
    std::vector<double> resid(n), part, delta, part5, delta5, ref5;
    for (int i = 0; i < n; i++) resid[i] = 0.05 * (i + 1) - 0.1;
    lm_partials_n(8, J8, resid, part);
    lm_solve_n(8, part, 0.01, delta);
    lm_partials_n(5, J5, resid, part5);
    lm_solve_n(5, part5, 0.01, delta5);
    compute_parameter_update_on_device(J5, resid, 0.01, ref5);
    if (part.size() != 73 || delta.size() != 8 || delta5 != ref5) { std::printf("FAIL LM functions\n"); fails++; }
    for (int bad : {0, 9}) {
        bool threw = false;
        try { lm_solve_n(bad, part, 0.01, delta5); } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL n_par = %d was accepted\n", bad); fails++; }
    }
    for (int i = 0; i < n; ++i) {
        std::printf("BASEP %d %a\nBASE %d %a\nJACP %d", i, basep[i], i, base8[i], i);
        for (int c = 0; c < 8; c++) std::printf(" %a", J8p[(size_t)i * 8 + c]);
        std::printf("\nJAC %d", i);
        for (int c = 0; c < 8; c++) std::printf(" %a", J8[(size_t)i * 8 + c]);
        std::printf("\n");
    }
    std::printf("PART 0");
    for (double x : part) std::printf(" %a", x);
    std::printf("\nDELTA 0");
    for (double x : delta) std::printf(" %a", x);
    std::printf("\n");
    std::printf(fails ? "FAILED (%d)\n" : "all C++ eight-column checks passed\n", fails);
    return fails ? 1 : 0;
}
