// C++ test of hadi_host::sample_ladder, compute_base_prices_samples and compute_jacobian_samples (include/hadi_host.hpp).
// One 50x25 batch of four puts with dividends, 20 steps, snapshots after steps 5, 12 and 20; every instance with its own six spots
// (S_0, another node, two interior off-node spots, one in the first and one in the last interval) and scales.  Prints every number
// as a hexadecimal double: tests/test_cpp_samples.py makes the same calls through the Python mirror and compares bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "hadi_host.hpp"

using namespace hadi_host;

int main() {
    const double S_0 = 100.0, V_0 = 0.04, T = 1.0, r_d = 0.025, r_f = 0.007, rho = -0.9, sigma = 0.3, kappa = 1.5, eta = 0.04;
    const double theta = 0.8;
    const int m1 = 50, m2 = 25, n = 4, N = 20, total_size = (m1 + 1) * (m2 + 1), n_samp = 6;
    const double delta_t = T / N;
    Handle h(0);
    PutStrikes strikes(n);
    for (int i = 0; i < n; ++i) strikes[i] = 90.0 + 5.0 * i;
    GridViews grids;
    buildMultipleGridViews(grids, n, m1, m2);
    std::vector<double> U_0((size_t)n * total_size);
    Samples per;  // [4][6]
    per.rows = n;
    for (int i = 0; i < n; ++i) {
        const double K = strikes[i];
        Grid g(m1, 8 * K, S_0, K, K / 5, m2, 5.0, V_0, 5.0 / 500);
        grids.set(i, g);
        for (int j = 0; j <= m2; j++)
            for (int k = 0; k <= m1; k++) U_0[(size_t)i * total_size + k + j * (m1 + 1)] = std::max(K - g.Vec_s[k], 0.0);
        const std::vector<double> &s = g.Vec_s;
        const double x[n_samp] = {S_0, s[7], s[16] + 0.37 * (s[17] - s[16]), s[33] + 0.5 * (s[34] - s[33]), s[0] + 0.4 * (s[1] - s[0]),
                                  s[m1 - 1] + 0.6 * (s[m1] - s[m1 - 1])};
        for (int q = 0; q < n_samp; q++) {
            per.spots.push_back(x[q]);
            per.scales.push_back(q == 0 ? 1.0 : 0.75 + 0.125 * q);
        }
    }
    Samples shared;  // one list for the batch, no scales
    shared.spots = {S_0, 61.7, 93.3, 127.4};
    const std::vector<int> snaps = {5, 12, 20};
    Dividends div{{0.2, 0.4, 0.6, 0.8}, {0.5, 0.3, 0.2, 0.1}, {0.02, 0.02, 0.02, 0.02}};
    int fails = 0;
    DO_Workspace ws(n, total_size);
    ws.U = U_0;
    std::vector<double> out, lad, shared_out, prices, J, base;
    sample_ladder(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, per, snaps, out,
                  HADI_DIV, nullptr, &div, &strikes);
    if (ws.U != U_0) { std::printf("FAIL the initial condition was modified\n"); fails++; }
    // the S_0 column (scale 1) is the maturity ladder, bit for bit
    maturity_ladder(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, snaps, lad,
                    HADI_DIV, nullptr, &div, &strikes);
    if (out.size() != (size_t)n * 3 * n_samp || lad.size() != (size_t)n * 3) { std::printf("FAIL sizes\n"); fails++; }
    for (int i = 0; i < n && !fails; i++)
        for (int q = 0; q < 3; q++)
            if (out[((size_t)i * 3 + q) * n_samp] != lad[(size_t)i * 3 + q]) { std::printf("FAIL the S_0 column is not the ladder (%d, %d)\n", i, q); fails++; }
    sample_ladder(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, shared, snaps,
                  shared_out, HADI_DIV, nullptr, &div, &strikes);
    if (shared_out.size() != (size_t)n * 3 * 4) { std::printf("FAIL shared size\n"); fails++; }
    compute_base_prices_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, per,
                                snaps, prices, HADI_DIV, nullptr, &div, &strikes);
    compute_jacobian_samples(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, U_0, per, snaps,
                             J, base, 1e-6, HADI_DIV, &div, &strikes);
    if (prices.size() != out.size() || base != prices || J.size() != out.size() * 5) { std::printf("FAIL launchers\n"); fails++; }
    for (int bad = 0; bad < 3; bad++) {  // a spot off the grid; a non-finite scale; a list that is not [rows][n_samp]
        Samples b = per;
        if (bad == 0) b.spots[7] = -1.0;
        else if (bad == 1) b.scales[3] = INFINITY;
        else b.spots.pop_back();
        bool threw = false;
        try {
            sample_ladder(h, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, n, grids, ws, b, snaps, lad,
                          HADI_DIV, nullptr, &div, &strikes);
        } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { std::printf("FAIL a bad sample list was accepted (%d)\n", bad); fails++; }
    }
    for (int i = 0; i < n; ++i)
        for (int q = 0; q < 3; q++) {
            std::printf("SAMP %d", i * 3 + q);
            for (int c = 0; c < n_samp; c++) std::printf(" %a", out[((size_t)i * 3 + q) * n_samp + c]);
            std::printf("\nSHARED %d", i * 3 + q);
            for (int c = 0; c < 4; c++) std::printf(" %a", shared_out[((size_t)i * 3 + q) * 4 + c]);
            std::printf("\nPRICE %d", i * 3 + q);
            for (int c = 0; c < n_samp; c++) std::printf(" %a", prices[((size_t)i * 3 + q) * n_samp + c]);
            std::printf("\n");
            for (int c = 0; c < n_samp; c++) {
                std::printf("JAC %d", (i * 3 + q) * n_samp + c);
                for (int z = 0; z < 5; z++) std::printf(" %a", J[(((size_t)i * 3 + q) * n_samp + c) * 5 + z]);
                std::printf("\n");
            }
        }
    std::printf(fails ? "FAILED (%d)\n" : "all C++ sample checks passed\n", fails);
    return fails ? 1 : 0;
}
