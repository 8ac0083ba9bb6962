// C++ test of hadi_host::bates_timestepping, compute_base_prices_bates and compute_jacobian_bates (include/hadi_host.hpp).
// One 50x25 batch of four puts with dividends, 20 steps, every instance with its own jump law (the third has intensity 0 and must
// equal its plain solve bit for bit), then the launchers with one shared law.  Prints every number as a hexadecimal double:
// tests/test_cpp_jumps.py makes the same calls through the Python mirror and compares bit for bit.
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
    Jumps none = shared;
    none.lambda = 0.0;
    int fails = 0;
    DO_Workspace field(n, total_size), ws(n, total_size), plain(n, total_size), empty(n, total_size);
    field.U = U_0; ws.U = U_0; plain.U = U_0; empty.U = U_0;
    bates_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, field, per, HADI_DIV, &div, &strikes);
    // zero intensity is the plain call, bit for bit
    bates_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, none, HADI_DIV, &div, &strikes);
    {
        hadi_problem p = detail::make(HADI_DIV, n, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, plain.U.data(),
                                      nullptr, &div, &strikes);
        detail::check(h, hadi_DO_timestepping(h.ctx, &p));
    }
    if (empty.U != plain.U) { std::printf("FAIL zero intensity is not the plain call\n"); fails++; }
    if (field.U == plain.U) { std::printf("FAIL the jumps changed nothing\n"); fails++; }
    {  // a zero-intensity instance inside a jump call is its plain solve on the kernels a jump call runs: the streaming ones
        DO_Workspace streamed(n, total_size);
        streamed.U = U_0;
        hadi_problem p = detail::make(HADI_DIV, n, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, streamed.U.data(),
                                      nullptr, &div, &strikes);
        detail::check(h, hadi_set_tuning(h.ctx, "small_grid", 0));
        detail::check(h, hadi_DO_timestepping(h.ctx, &p));
        detail::check(h, hadi_set_tuning(h.ctx, "small_grid", 1));
        if (!std::equal(field.U.begin() + 2 * (size_t)total_size, field.U.begin() + 3 * (size_t)total_size,
                        streamed.U.begin() + 2 * (size_t)total_size)) {
            std::printf("FAIL the zero-intensity instance is not its plain solve\n");
            fails++;
        }
    }
    std::vector<double> prices, J, base;
    compute_base_prices_bates(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws,
                              shared, prices, HADI_DIV, &div, &strikes);
    compute_jacobian_bates(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                           shared, J, base, 1e-6, HADI_DIV, &div, &strikes);
    if (prices.size() != (size_t)n || base != prices || J.size() != (size_t)n * 5) { std::printf("FAIL launchers\n"); fails++; }
    for (int bad = 0; bad < 3; bad++) {  // a negative intensity; a jump volatility of zero; a broken shared-grid promise
        Jumps b = per;
        if (bad == 0) b.lambda_i[1] = -0.5;
        else if (bad == 1) b.sigma_i[3] = 0.0;
        else { b = shared; b.shared_grid = true; }
        bool threw = false;
        try {
            bates_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, b, HADI_DIV, &div, &strikes);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL a bad jump description was accepted (%d)\n", bad); fails++; }
    }
    for (int i = 0; i < n; ++i) {
        std::printf("FIELD %d", i);
        for (int c = 0; c < total_size; c += 97) std::printf(" %a", field.U[(size_t)i * total_size + c]);
        std::printf("\nPRICE %d %a\nJAC %d", i, prices[i], i);
        for (int c = 0; c < 5; c++) std::printf(" %a", J[(size_t)i * 5 + c]);
        std::printf("\n");
    }
    std::printf(fails ? "FAILED (%d)\n" : "all C++ jump checks passed\n", fails);
    return fails ? 1 : 0;
}
