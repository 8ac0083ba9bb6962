// C++ test of hadi_host::compute_greeks (include/hadi_host.hpp).  One 50x25 batch of four American puts with dividends, 20
// steps, the grids and payoffs of the reference's own device test (src/device_solver.cpp:677, 711-715).  Prints every number
// as a hexadecimal double: tests/test_cpp_greeks.py makes the same call through the Python mirror and compares bit for bit.
#include <algorithm>
#include <cstdio>

#include "hadi_host.hpp"

using namespace hadi_host;

int main() {
    const double S_0 = 100.0, V_0 = 0.04, T = 1.0, r_d = 0.025, r_f = 0.007, rho = -0.9, sigma = 0.3, kappa = 1.5, eta = 0.04;
    const double theta = 0.8;
    const int m1 = 50, m2 = 25, n = 4, N = 20, total_size = (m1 + 1) * (m2 + 1);
    const double delta_t = T / N;
    Handle h(0);
    PutStrikes strikes(n);
    for (int i = 0; i < n; ++i) strikes[i] = 90.0 + 5.0 * i;
    GridViews grids;
    buildMultipleGridViews(grids, n, m1, m2);
    DO_Workspace workspace(n, total_size);
    for (int i = 0; i < n; ++i) {
        const double K = strikes[i];
        Grid g(m1, 8 * K, S_0, K, K / 5, m2, 5.0, V_0, 5.0 / 500);
        grids.set(i, g);
        for (int j = 0; j <= m2; j++)
            for (int k = 0; k <= m1; k++) workspace.U[(size_t)i * total_size + k + j * (m1 + 1)] = std::max(K - g.Vec_s[k], 0.0);
    }
    const std::vector<double> U_before = workspace.U;
    Dividends div{{0.2, 0.4, 0.6, 0.8}, {0.5, 0.3, 0.2, 0.1}, {0.02, 0.02, 0.02, 0.02}};
    std::vector<double> greeks, ladder, greeks_only;
    compute_greeks(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, workspace,
                   greeks, &ladder, HADI_AM_DIV, nullptr, &div, &strikes);
    compute_greeks(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, workspace,
                   greeks_only, nullptr, HADI_AM_DIV, nullptr, &div, &strikes);
    int fails = 0;
    if (workspace.U != U_before) { std::printf("FAIL workspace.U was written\n"); fails++; }
    if (greeks_only != greeks) { std::printf("FAIL the node row depends on the ladder argument\n"); fails++; }
    if (greeks.size() != (size_t)n * HADI_N_GREEKS || ladder.size() != (size_t)n * (m1 + 1) * HADI_N_GREEKS) { std::printf("FAIL sizes\n"); fails++; }
    for (int i = 0; i < n; ++i) {
        std::printf("GREEKS %d", i);
        for (int c = 0; c < HADI_N_GREEKS; c++) std::printf(" %a", greeks[(size_t)i * HADI_N_GREEKS + c]);
        std::printf("\n");
    }
    std::printf(fails ? "FAILED (%d)\n" : "all C++ Greeks checks passed\n", fails);
    return fails ? 1 : 0;
}
