// C++ test of hadi_host::cliquet_timestepping, compute_base_prices_cliquet and compute_jacobian_cliquet (include/hadi_host.hpp).
// One 50x25 batch of four puts with dividends, 20 steps, every instance with its own reference node, mode, fixing schedule and
// weights (rows zero-padded; the first fixes at the end of step 8, which pays a dividend at its start, and at the valuation date).
// Prints every number as a hexadecimal double: tests/test_cpp_cliquet.py makes the same calls through the Python mirror and
// compares bit for bit.
#include <algorithm>
#include <cstdio>

#include "hadi_host.hpp"

using namespace hadi_host;

int main() {
    const double S_0 = 100.0, V_0 = 0.04, T = 1.0, r_d = 0.025, r_f = 0.007, rho = -0.9, sigma = 0.3, kappa = 1.5, eta = 0.04;
    const double theta = 0.8;
    const int m1 = 50, m2 = 25, n = 4, N = 20, total_size = (m1 + 1) * (m2 + 1);
    const double delta_t = T / N;
    const int node[4] = {20, 25, 30, 22};
    Handle h(0);
    PutStrikes strikes(n);
    for (int i = 0; i < n; ++i) strikes[i] = 90.0 + 5.0 * i;
    GridViews grids;
    buildMultipleGridViews(grids, n, m1, m2);
    std::vector<double> U_0((size_t)n * total_size);
    Cliquet per;  // [4][3]
    per.ref_spot.resize(n);
    for (int i = 0; i < n; ++i) {
        const double K = strikes[i];
        Grid g(m1, 8 * K, S_0, K, K / 5, m2, 5.0, V_0, 5.0 / 500);
        grids.set(i, g);
        per.ref_spot[i] = g.Vec_s[node[i]];
        for (int j = 0; j <= m2; j++)
            for (int k = 0; k <= m1; k++) U_0[(size_t)i * total_size + k + j * (m1 + 1)] = std::max(K - g.Vec_s[k], 0.0);
    }
    Dividends div{{0.2, 0.4, 0.6, 0.8}, {0.5, 0.3, 0.2, 0.1}, {0.02, 0.02, 0.02, 0.02}};
    per.mode = {HADI_FIX_SHARES, HADI_FIX_RETURN, HADI_FIX_RETURN, HADI_FIX_SHARES};
    per.fix_steps = {8, 16, 20, 5, 10, 0, 0, 0, 0, 20, 0, 0};
    per.weights = {0.0, 1.0, 0.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0};
    per.fix_rows = n;
    Cliquet shared;  // SHARES, no weights, one schedule
    shared.ref_spot = per.ref_spot;
    shared.fix_steps = {5, 10, 15, 20};
    Cliquet none = per;
    none.fix_steps.clear();
    none.weights.clear();
    none.fix_rows = 1;
    int fails = 0;
    DO_Workspace field(n, total_size), ws(n, total_size), plain(n, total_size), empty(n, total_size);
    field.U = U_0; ws.U = U_0; plain.U = U_0; empty.U = U_0;
    cliquet_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, field, per, HADI_DIV, &div, &strikes);
    // an empty schedule is the plain call, bit for bit
    cliquet_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, none, HADI_DIV, &div, &strikes);
    {
        hadi_problem p = detail::make(HADI_DIV, n, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, plain.U.data(),
                                      nullptr, &div, &strikes);
        detail::check(h, hadi_DO_timestepping(h.ctx, &p));
    }
    if (empty.U != plain.U) { std::printf("FAIL the empty schedule is not the plain call\n"); fails++; }
    if (field.U == plain.U) { std::printf("FAIL the fixings changed nothing\n"); fails++; }
    std::vector<double> prices, J, base;
    compute_base_prices_cliquet(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws,
                                shared, prices, HADI_DIV, &div, &strikes);
    compute_jacobian_cliquet(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0,
                             shared, J, base, 1e-6, HADI_DIV, &div, &strikes);
    if (prices.size() != (size_t)n || base != prices || J.size() != (size_t)n * 5) { std::printf("FAIL launchers\n"); fails++; }
    for (int bad = 0; bad < 3; bad++) {  // a date behind the last step; a mode that is none; a reference spot between two nodes
        Cliquet q = per;
        if (bad == 0) q.fix_steps[2] = 21;
        else if (bad == 1) q.mode[1] = 2;
        else q.ref_spot[2] += 0.01;
        bool threw = false;
        try {
            cliquet_timestepping(h, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, n, grids, empty, q, HADI_DIV, &div, &strikes);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL a bad cliquet description was accepted (%d)\n", bad); fails++; }
    }
    for (int i = 0; i < n; ++i) {
        std::printf("FIELD %d", i);
        for (int c = 0; c < total_size; c += 97) std::printf(" %a", field.U[(size_t)i * total_size + c]);
        std::printf("\nPRICE %d %a\nJAC %d", i, prices[i], i);
        for (int c = 0; c < 5; c++) std::printf(" %a", J[(size_t)i * 5 + c]);
        std::printf("\n");
    }
    std::printf(fails ? "FAILED (%d)\n" : "all C++ cliquet checks passed\n", fails);
    return fails ? 1 : 0;
}
