// C++ test of hadi_host::barrier_timestepping, compute_base_prices_barrier and compute_jacobian_barrier (include/hadi_host.hpp).
// One 50x25 batch of four puts with dividends, 20 steps, every instance with its own barriers, rebate and monitoring schedule (rows
// zero-padded; the first is monitored at the end of step 8, which pays a dividend at its start, and at the valuation date).  Prints
// every number as a hexadecimal double: tests/test_cpp_barrier.py makes the same calls through the Python mirror and compares
// bit for bit.
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
    Barrier per;  // [4][3]
    per.lower = {63.0, 76.0, 60.0, 78.75};
    per.upper = {117.0, 114.0, 140.0, 131.25};
    per.rebate = {0.0, 1.5, 0.25, 3.0};
    per.mon_steps = {8, 16, 20, 5, 10, 0, 0, 0, 0, 20, 0, 0};
    per.mon_rows = n;
    Barrier shared;  // up-and-out, no rebate, one schedule
    shared.upper = {117.0, 114.0, 140.0, 131.25};
    shared.mon_steps = {5, 10, 15, 20};
    Barrier none = per;
    none.mon_steps.clear();
    none.mon_rows = 1;
    int fails = 0;
    DO_Workspace field(n, total_size), ws(n, total_size), plain(n, total_size), empty(n, total_size);
    field.U = U_0; ws.U = U_0; plain.U = U_0; empty.U = U_0;
    barrier_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, field, per, HADI_DIV, &div, &strikes);
    // an empty schedule is the plain call, bit for bit
    barrier_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, none, HADI_DIV, &div, &strikes);
    {
        hadi_problem p = detail::make(HADI_DIV, n, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, plain.U.data(),
                                      nullptr, &div, &strikes);
        detail::check(h, hadi_DO_timestepping(h.ctx, &p));
    }
    if (empty.U != plain.U) { std::printf("FAIL the empty schedule is not the plain call\n"); fails++; }
    if (field.U == plain.U) { std::printf("FAIL the barrier changed nothing\n"); fails++; }
    std::vector<double> prices, J, base;
    compute_base_prices_barrier(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws,
                                shared, prices, HADI_DIV, &div, &strikes);
    compute_jacobian_barrier(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                             shared, J, base, 1e-6, HADI_DIV, &div, &strikes);
    if (prices.size() != (size_t)n || base != prices || J.size() != (size_t)n * 5) { std::printf("FAIL launchers\n"); fails++; }
    for (int bad = 0; bad < 2; bad++) {  // a date behind the last step; a lower barrier above the upper one
        Barrier b = per;
        if (bad == 0) b.mon_steps[2] = 21;
        else std::swap(b.lower, b.upper);
        bool threw = false;
        try {
            barrier_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, b, HADI_DIV, &div, &strikes);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL a bad barrier description was accepted (%d)\n", bad); fails++; }
    }
    for (int i = 0; i < n; ++i) {
        std::printf("FIELD %d", i);
        for (int c = 0; c < total_size; c += 97) std::printf(" %a", field.U[(size_t)i * total_size + c]);
        std::printf("\nPRICE %d %a\nJAC %d", i, prices[i], i);
        for (int c = 0; c < 5; c++) std::printf(" %a", J[(size_t)i * 5 + c]);
        std::printf("\n");
    }
    std::printf(fails ? "FAILED (%d)\n" : "all C++ barrier checks passed\n", fails);
    return fails ? 1 : 0;
}
