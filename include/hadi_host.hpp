// hadi_host.hpp -- C++ host mirror of the reference's launcher interface on top of the C ABI (include/hadi.h).
//
// The reference (BCW-dot/PDE-based-Heston-Solver-GPU-accelerated) is C++ on Kokkos; Kokkos is not available in this
// image, so this header offers the same host-callable entry points -- same names, same argument order and meaning --
// over std::vector / raw pointers instead of Kokkos::View, header-only, no dependency besides libhadi:
//
//   Grid                                   Grid::Grid                        src/grid.cpp:16-61
//   GridViews / buildMultipleGridViews     grid_pod.hpp:8-111                (the four arrays of a batch, [n][len])
//   DO_Workspace                           DO_solver_workspace.hpp:4-44      (only U and lambda_bar cross the boundary)
//   parallel_DO_solve                      device_solver.hpp:52-185
//   compute_base_prices{,_american,_dividends,_american_dividends}   jacobian_computation.cpp:368, 629, 922, 1232
//   compute_jacobian{,_american,_dividends,_american_dividends}      jacobian_computation.cpp:204, 457, 726, 1031
//   compute_parameter_update_on_device                               jacobian_computation.cpp:107-195
//
// Arguments of the reference that only carried scratch (A0/A1/A2 solver arrays, bounds_d) do not exist here; failures
// throw std::runtime_error with the library's message (the reference's launchers return void).  With Kokkos present a
// maintainer binds View::data() pointers instead -- INTEGRATION.md shows that shim.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "hadi.h"

namespace hadi_host {

struct Handle {  // one per process and GPU, next to Kokkos::initialize in the reference's main()
    hadi_ctx *ctx = nullptr;
    explicit Handle(int device = 0) {
        const int rc = hadi_create(&ctx, device);
        if (rc) throw std::runtime_error(std::string("hadi_create: ") + hadi_status_string(rc));
    }
    ~Handle() { hadi_destroy(ctx); }
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
};

// src/grid.cpp:16-61 (same constructor arguments)
struct Grid {
    int m1, m2;
    std::vector<double> Vec_s, Vec_v, Delta_s, Delta_v;
    Grid(int m1_, double S, double S_0, double K, double c, int m2_, double V, double V_0, double d)
        : m1(m1_), m2(m2_), Vec_s(m1_ + 1), Vec_v(m2_ + 1), Delta_s(m1_), Delta_v(m2_) {
        if (hadi_make_grid(m1, S, S_0, K, c, m2, V, V_0, d, Vec_s.data(), Vec_v.data(), Delta_s.data(), Delta_v.data()))
            throw std::runtime_error("hadi_make_grid failed");
    }
};

// grid_pod.hpp:8-111: the GridViews of a batch as four [nInstances][len] host arrays
struct GridViews {
    int nInstances = 0, m1 = 0, m2 = 0;
    std::vector<double> Vec_s, Vec_v, Delta_s, Delta_v;
    void set(int i, const Grid &g) {
        std::copy(g.Vec_s.begin(), g.Vec_s.end(), Vec_s.begin() + (size_t)i * (m1 + 1));
        std::copy(g.Vec_v.begin(), g.Vec_v.end(), Vec_v.begin() + (size_t)i * (m2 + 1));
        std::copy(g.Delta_s.begin(), g.Delta_s.end(), Delta_s.begin() + (size_t)i * m1);
        std::copy(g.Delta_v.begin(), g.Delta_v.end(), Delta_v.begin() + (size_t)i * m2);
    }
};
inline void buildMultipleGridViews(GridViews &grids, int nInstances, int m1, int m2) {
    grids.nInstances = nInstances; grids.m1 = m1; grids.m2 = m2;
    grids.Vec_s.assign((size_t)nInstances * (m1 + 1), 0.0);
    grids.Vec_v.assign((size_t)nInstances * (m2 + 1), 0.0);
    grids.Delta_s.assign((size_t)nInstances * m1, 0.0);
    grids.Delta_v.assign((size_t)nInstances * m2, 0.0);
}

// DO_solver_workspace.hpp:4-44
struct DO_Workspace {
    int nInstances, total_size;
    std::vector<double> U, lambda_bar;  // [nInstances][total_size]
    DO_Workspace(int n, int total) : nInstances(n), total_size(total), U((size_t)n * total, 0.0), lambda_bar((size_t)n * total, 0.0) {}
};

struct Dividends {  // device_solver.hpp:409-413
    std::vector<double> dates, amounts, percentages;
};

// Put boundary data (hadi.h, enum hadi_option_type) -- NOT in the reference, whose only boundary class is call-specific
// (BoundaryConditions.hpp:7-12).  Passing the strikes as the optional last argument of a launcher below switches the batch
// to the put's boundary values; the caller supplies the put payoff in workspace.U / U_0 as usual.
using PutStrikes = std::vector<double>;

namespace detail {
inline hadi_problem make(int variant, int n, int m1, int m2, int N, double delta_t, double theta, double r_d, double r_f,
                         double rho, double sigma, double kappa, double eta, const GridViews &g, double *U,
                         const double *U_0, const Dividends *div, const PutStrikes *put = nullptr) {
    if (g.nInstances != n || g.m1 != m1 || g.m2 != m2) throw std::runtime_error("grid batch does not match (n, m1, m2)");
    hadi_problem p{};
    if (put) {
        if ((int)put->size() != n) throw std::runtime_error("put strikes do not match the batch");
        p.option_type = HADI_PUT;
        p.strike_i = put->data();
    }
    p.n_instances = n; p.m1 = m1; p.m2 = m2; p.variant = variant; p.memspace = HADI_MEM_HOST;
    p.N = N; p.delta_t = delta_t; p.theta = theta;
    p.r_d = r_d; p.r_f = r_f; p.rho = rho; p.sigma = sigma; p.kappa = kappa; p.eta = eta;
    p.vec_s = g.Vec_s.data(); p.vec_v = g.Vec_v.data(); p.delta_s = g.Delta_s.data(); p.delta_v = g.Delta_v.data();
    p.U = U; p.U_0 = U_0;
    if (div) {
        p.num_dividends = (int)div->dates.size();
        p.dividend_dates = div->dates.data(); p.dividend_amounts = div->amounts.data();
        p.dividend_percentages = div->percentages.data();
    }
    return p;
}
inline void check(const Handle &h, int rc) {
    if (rc) throw std::runtime_error(hadi_last_error(h.ctx));
}
}  // namespace detail

// device_solver.hpp:52-185 (S_0, V_0 are doubles here; the reference declares them int, :56-57)
inline void parallel_DO_solve(Handle &h, int nInstances, double S_0, double V_0, int m1, int m2, int N, double /*T*/,
                              double delta_t, double theta, double r_d, double r_f, double rho, double sigma, double kappa,
                              double eta, const GridViews &deviceGrids, DO_Workspace &workspace, std::vector<double> &base_prices,
                              const PutStrikes *put = nullptr) {
    base_prices.resize(nInstances);
    hadi_problem p = detail::make(HADI_EU, nInstances, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, nullptr, put);
    detail::check(h, hadi_parallel_DO_solve(h.ctx, &p, S_0, V_0, base_prices.data()));
}

// jacobian_computation.cpp:368-448 and the three variants; workspace.U holds the initial condition (the reference's
// callers do deep_copy(workspace.U, U_0) first, heston_calibration.cpp:216)
inline void compute_base_prices(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                double delta_t, int num_strikes, const GridViews &deviceGrids, DO_Workspace &workspace,
                                std::vector<double> &base_prices) {
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(HADI_EU, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, nullptr);
    detail::check(h, hadi_compute_base_prices(h.ctx, &p, S_0, V_0, base_prices.data()));
}
inline void compute_base_prices_american(Handle &h, double S_0, double V_0, double, double r_d, double r_f, double rho,
                                         double sigma, double kappa, double eta, int m1, int m2, int, int N, double theta,
                                         double delta_t, int num_strikes, const GridViews &deviceGrids,
                                         const std::vector<double> &U_0, DO_Workspace &workspace,
                                         std::vector<double> &base_prices) {
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(HADI_AM, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), U_0.data(), nullptr);
    p.lambda_bar = workspace.lambda_bar.data();
    detail::check(h, hadi_compute_base_prices_american(h.ctx, &p, S_0, V_0, base_prices.data()));
}
inline void compute_base_prices_dividends(Handle &h, double S_0, double V_0, double, double r_d, double r_f, double rho,
                                          double sigma, double kappa, double eta, int m1, int m2, int, int N, double theta,
                                          double delta_t, int num_strikes, const GridViews &deviceGrids, DO_Workspace &workspace,
                                          const Dividends &div, std::vector<double> &base_prices) {
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(HADI_DIV, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, &div);
    detail::check(h, hadi_compute_base_prices_dividends(h.ctx, &p, S_0, V_0, base_prices.data()));
}
inline void compute_base_prices_american_dividends(Handle &h, double S_0, double V_0, double, double r_d, double r_f,
                                                   double rho, double sigma, double kappa, double eta, int m1, int m2, int,
                                                   int N, double theta, double delta_t, int num_strikes,
                                                   const GridViews &deviceGrids, const std::vector<double> &U_0,
                                                   DO_Workspace &workspace, const Dividends &div,
                                                   std::vector<double> &base_prices, const PutStrikes *put = nullptr) {
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(HADI_AM_DIV, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta,
                                  deviceGrids, workspace.U.data(), U_0.data(), &div, put);
    p.lambda_bar = workspace.lambda_bar.data();
    detail::check(h, hadi_compute_base_prices_american_dividends(h.ctx, &p, S_0, V_0, base_prices.data()));
}

// Greeks at (S_0, V_0) and, with `ladder`, the spot ladder of the v-row of V_0 (hadi_compute_greeks; NOT in the reference).
// greeks: [num_strikes][HADI_N_GREEKS], ladder: [num_strikes][m1+1][HADI_N_GREEKS], columns enum hadi_greek.  workspace.U holds
// the initial condition and is not modified; U_0 (American variants) defaults to it.
inline void compute_greeks(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                           double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta, double delta_t,
                           int num_strikes, const GridViews &deviceGrids, const DO_Workspace &workspace,
                           std::vector<double> &greeks, std::vector<double> *ladder = nullptr, int variant = HADI_EU,
                           const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr,
                           const PutStrikes *put = nullptr) {
    greeks.resize((size_t)num_strikes * HADI_N_GREEKS);
    if (ladder) ladder->resize((size_t)num_strikes * (m1 + 1) * HADI_N_GREEKS);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_compute_greeks(h.ctx, &p, S_0, V_0, greeks.data(), ladder ? ladder->data() : nullptr));
}

// Maturity ladder (hadi_maturity_ladder and its two launchers; NOT in the reference): the price node after each of the steps
// snap_steps (strictly increasing, within 1..N) of ONE N-step sweep -- prices: [num_strikes][snap_steps.size()], entry q what
// the same call with N = snap_steps[q] returns.  workspace.U holds the initial condition and is not modified.
inline void maturity_ladder(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                            double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta, double delta_t,
                            int num_strikes, const GridViews &deviceGrids, const DO_Workspace &workspace,
                            const std::vector<int> &snap_steps, std::vector<double> &prices, int variant = HADI_EU,
                            const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr,
                            const PutStrikes *put = nullptr) {
    prices.resize((size_t)num_strikes * snap_steps.size());
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_maturity_ladder(h.ctx, &p, S_0, V_0, (int)snap_steps.size(), snap_steps.data(), prices.data()));
}
// ... with the v-grid rebuilt for V_0, as compute_base_prices does
inline void compute_base_prices_ladder(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                       double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N,
                                       double theta, double delta_t, int num_strikes, const GridViews &deviceGrids,
                                       const DO_Workspace &workspace, const std::vector<int> &snap_steps,
                                       std::vector<double> &prices, int variant = HADI_EU, const std::vector<double> *U_0 = nullptr,
                                       const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    prices.resize((size_t)num_strikes * snap_steps.size());
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_ladder(h.ctx, &p, S_0, V_0, (int)snap_steps.size(), snap_steps.data(), prices.data()));
}
// J: [num_strikes][snap_steps.size()][5], base_prices: [num_strikes][snap_steps.size()]
inline void compute_jacobian_ladder(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                                    double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                    double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                    const std::vector<int> &snap_steps, std::vector<double> &J, std::vector<double> &base_prices,
                                    double eps = 1e-6, int variant = HADI_EU, const Dividends *div = nullptr,
                                    const PutStrikes *put = nullptr) {
    J.resize((size_t)num_strikes * snap_steps.size() * 5);
    base_prices.resize((size_t)num_strikes * snap_steps.size());
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_ladder(h.ctx, &p, S_0, V_0, eps, (int)snap_steps.size(), snap_steps.data(), J.data(),
                                                  base_prices.data()));
}

// Sampled ladder (hadi_sample_ladder and its two launchers; NOT in the reference): the ladder's calls with the state of the v-row
// of V_0 evaluated at arbitrary spots where the ladder copies the node of S_0 (hadi.h states the interpolant).  spots / scales:
// [rows][spots.size() / rows], rows = 1 (one list for the batch) or num_strikes; scales empty = 1.
struct Samples {
    std::vector<double> spots, scales;
    int rows = 1;
    hadi_samples view() const {
        if (rows < 1 || spots.empty() || spots.size() % (size_t)rows) throw std::runtime_error("spots is not [rows][n_samp]");
        if (!scales.empty() && scales.size() != spots.size()) throw std::runtime_error("scales does not have the shape of spots");
        return hadi_samples{(int)(spots.size() / rows), spots.data(), scales.empty() ? nullptr : scales.data(), rows};
    }
};
// out: [num_strikes][snap_steps.size()][n_samp].  workspace.U holds the initial condition and is not modified.
inline void sample_ladder(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma, double kappa,
                          double eta, int m1, int m2, int /*total_size*/, int N, double theta, double delta_t, int num_strikes,
                          const GridViews &deviceGrids, const DO_Workspace &workspace, const Samples &samples,
                          const std::vector<int> &snap_steps, std::vector<double> &out, int variant = HADI_EU,
                          const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    out.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_sample_ladder(h.ctx, &p, V_0, &s, (int)snap_steps.size(), snap_steps.data(), out.data()));
}
// ... with the v-grid rebuilt for V_0, as compute_base_prices does
inline void compute_base_prices_samples(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                                        double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                        double delta_t, int num_strikes, const GridViews &deviceGrids, const DO_Workspace &workspace,
                                        const Samples &samples, const std::vector<int> &snap_steps, std::vector<double> &out,
                                        int variant = HADI_EU, const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr,
                                        const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    out.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_samples(h.ctx, &p, V_0, &s, (int)snap_steps.size(), snap_steps.data(), out.data()));
}
// J: [num_strikes][snap_steps.size()][n_samp][5], base: [num_strikes][snap_steps.size()][n_samp]
inline void compute_jacobian_samples(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma, double kappa,
                                     double eta, int m1, int m2, int /*total_size*/, int N, double theta, double delta_t,
                                     int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                     const Samples &samples, const std::vector<int> &snap_steps, std::vector<double> &J,
                                     std::vector<double> &base, double eps = 1e-6, int variant = HADI_EU,
                                     const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    J.resize((size_t)num_strikes * snap_steps.size() * s.n_samp * 5);
    base.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_samples(h.ctx, &p, V_0, eps, &s, (int)snap_steps.size(), snap_steps.data(), J.data(),
                                                   base.data()));
}

// Bermudan options (hadi_bermudan_timestepping and its two launchers; NOT in the reference): the European or dividend sweep with
// U <- max(U, payoff) at the end of the listed steps.  ex_steps: [ex_rows][ex_steps.size() / ex_rows], ex_rows = 1 (one schedule
// for the batch) or num_strikes (rows strictly increasing within 1..N, zero-padded).  The payoff is U_0, or the initial
// workspace.U where U_0 is null; workspace.U receives the field.
inline void bermudan_timestepping(Handle &h, int m1, int m2, int N, double delta_t, double theta, double r_d, double r_f, double rho,
                                  double sigma, double kappa, double eta, int num_strikes, const GridViews &deviceGrids,
                                  DO_Workspace &workspace, const std::vector<int> &ex_steps, int ex_rows = 1, int variant = HADI_EU,
                                  const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr,
                                  const PutStrikes *put = nullptr) {
    if (ex_rows < 1 || ex_steps.size() % (size_t)ex_rows) throw std::runtime_error("ex_steps is not [ex_rows][n_ex]");
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_bermudan_timestepping(h.ctx, &p, (int)(ex_steps.size() / ex_rows), ex_steps.data(), ex_rows));
}
// ... with the v-grid rebuilt for V_0 and the price pick, as compute_base_prices does
inline void compute_base_prices_bermudan(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                         double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N,
                                         double theta, double delta_t, int num_strikes, const GridViews &deviceGrids,
                                         DO_Workspace &workspace, const std::vector<int> &ex_steps, std::vector<double> &base_prices,
                                         int ex_rows = 1, int variant = HADI_EU, const std::vector<double> *U_0 = nullptr,
                                         const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    if (ex_rows < 1 || ex_steps.size() % (size_t)ex_rows) throw std::runtime_error("ex_steps is not [ex_rows][n_ex]");
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_bermudan(h.ctx, &p, S_0, V_0, (int)(ex_steps.size() / ex_rows), ex_steps.data(), ex_rows,
                                                       base_prices.data()));
}
// J: [num_strikes][5], base_prices: [num_strikes]; the six solves of an instance share its schedule
inline void compute_jacobian_bermudan(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                      double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                      double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                      const std::vector<int> &ex_steps, std::vector<double> &J, std::vector<double> &base_prices,
                                      double eps = 1e-6, int ex_rows = 1, int variant = HADI_EU, const Dividends *div = nullptr,
                                      const PutStrikes *put = nullptr) {
    if (ex_rows < 1 || ex_steps.size() % (size_t)ex_rows) throw std::runtime_error("ex_steps is not [ex_rows][n_ex]");
    J.resize((size_t)num_strikes * 5);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_bermudan(h.ctx, &p, S_0, V_0, eps, (int)(ex_steps.size() / ex_rows), ex_steps.data(), ex_rows,
                                                    J.data(), base_prices.data()));
}

// Discretely monitored knock-out barriers (hadi_barrier_timestepping and its two launchers; NOT in the reference): the European or
// dividend sweep with U <- rebate on the nodes at or beyond a barrier (s <= lower or s >= upper) at the end of the monitoring
// steps.  lower / upper / rebate: one value per instance, or empty = no barrier on that side / no rebate.  mon_steps:
// [mon_rows][mon_steps.size() / mon_rows], the rules of ex_steps above.  workspace.U is the caller's initial condition
// (monitoring at maturity is applied to it by the caller) and receives the field.
struct Barrier {
    std::vector<double> lower, upper, rebate;
    std::vector<int> mon_steps;
    int mon_rows = 1;
    hadi_barrier view(int num_strikes) const {
        if (mon_rows < 1 || mon_steps.size() % (size_t)mon_rows) throw std::runtime_error("mon_steps is not [mon_rows][n_mon]");
        for (const std::vector<double> *a : {&lower, &upper, &rebate})
            if (!a->empty() && a->size() != (size_t)num_strikes) throw std::runtime_error("a barrier array is not [num_strikes]");
        return hadi_barrier{lower.empty() ? nullptr : lower.data(), upper.empty() ? nullptr : upper.data(),
                            rebate.empty() ? nullptr : rebate.data(), (int)(mon_steps.size() / mon_rows), mon_steps.data(), mon_rows};
    }
};
inline void barrier_timestepping(Handle &h, int m1, int m2, int N, double delta_t, double theta, double r_d, double r_f, double rho,
                                 double sigma, double kappa, double eta, int num_strikes, const GridViews &deviceGrids,
                                 DO_Workspace &workspace, const Barrier &barrier, int variant = HADI_EU, const Dividends *div = nullptr,
                                 const PutStrikes *put = nullptr) {
    const hadi_barrier b = barrier.view(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_barrier_timestepping(h.ctx, &p, &b));
}
// ... with the v-grid rebuilt for V_0 and the price pick, as compute_base_prices does
inline void compute_base_prices_barrier(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                        double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N,
                                        double theta, double delta_t, int num_strikes, const GridViews &deviceGrids,
                                        DO_Workspace &workspace, const Barrier &barrier, std::vector<double> &base_prices,
                                        int variant = HADI_EU, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_barrier b = barrier.view(num_strikes);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_barrier(h.ctx, &p, S_0, V_0, &b, base_prices.data()));
}
// J: [num_strikes][5], base_prices: [num_strikes]; the six solves of an instance share its barriers, rebate and schedule
inline void compute_jacobian_barrier(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                     double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                     double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                     const Barrier &barrier, std::vector<double> &J, std::vector<double> &base_prices,
                                     double eps = 1e-6, int variant = HADI_EU, const Dividends *div = nullptr,
                                     const PutStrikes *put = nullptr) {
    const hadi_barrier b = barrier.view(num_strikes);
    J.resize((size_t)num_strikes * 5);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_barrier(h.ctx, &p, S_0, V_0, eps, &b, J.data(), base_prices.data()));
}

// Forward-start options and cliquets (hadi_cliquet_timestepping and its two launchers; NOT in the reference): the European or
// dividend sweep with U(i, j) <- a_i U(i_ref, j) + w P(i, j) at the end of the fixing steps.  ref_spot: one value per instance (a
// node of its s-grid); mode: one HADI_FIX_SHARES / HADI_FIX_RETURN per instance, or empty = SHARES; fix_steps:
// [fix_rows][fix_steps.size() / fix_rows], the rules of ex_steps above; weights: the same shape, or empty = 0.  workspace.U is the
// caller's initial condition and the payoff P (the launchers' U_0 likewise) and receives the field.
struct Cliquet {
    std::vector<double> ref_spot, weights;
    std::vector<int> mode, fix_steps;
    int fix_rows = 1;
    hadi_cliquet view(int num_strikes) const {
        if (fix_rows < 1 || fix_steps.size() % (size_t)fix_rows) throw std::runtime_error("fix_steps is not [fix_rows][n_fix]");
        if (!weights.empty() && weights.size() != fix_steps.size()) throw std::runtime_error("weights is not [fix_rows][n_fix]");
        if (ref_spot.size() != (size_t)num_strikes || (!mode.empty() && mode.size() != (size_t)num_strikes))
            throw std::runtime_error("a cliquet array is not [num_strikes]");
        return hadi_cliquet{ref_spot.data(), mode.empty() ? nullptr : mode.data(), (int)(fix_steps.size() / fix_rows), fix_steps.data(),
                            fix_rows, weights.empty() ? nullptr : weights.data()};
    }
};
inline void cliquet_timestepping(Handle &h, int m1, int m2, int N, double delta_t, double theta, double r_d, double r_f, double rho,
                                 double sigma, double kappa, double eta, int num_strikes, const GridViews &deviceGrids,
                                 DO_Workspace &workspace, const Cliquet &cliquet, int variant = HADI_EU, const Dividends *div = nullptr,
                                 const PutStrikes *put = nullptr) {
    const hadi_cliquet q = cliquet.view(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_cliquet_timestepping(h.ctx, &p, &q));
}
// ... with the v-grid rebuilt for V_0 and the price pick, as compute_base_prices does
inline void compute_base_prices_cliquet(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                        double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N,
                                        double theta, double delta_t, int num_strikes, const GridViews &deviceGrids,
                                        DO_Workspace &workspace, const Cliquet &cliquet, std::vector<double> &base_prices,
                                        int variant = HADI_EU, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_cliquet q = cliquet.view(num_strikes);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_cliquet(h.ctx, &p, S_0, V_0, &q, base_prices.data()));
}
// J: [num_strikes][5], base_prices: [num_strikes]; the six solves of an instance share its reference spot, mode, schedule and weights
inline void compute_jacobian_cliquet(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                     double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                     double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                     const Cliquet &cliquet, std::vector<double> &J, std::vector<double> &base_prices,
                                     double eps = 1e-6, int variant = HADI_EU, const Dividends *div = nullptr,
                                     const PutStrikes *put = nullptr) {
    const hadi_cliquet q = cliquet.view(num_strikes);
    J.resize((size_t)num_strikes * 5);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_cliquet(h.ctx, &p, S_0, V_0, eps, &q, J.data(), base_prices.data()));
}

// The Bates model (hadi_bates_timestepping and its two launchers; NOT in the reference): the European or dividend sweep with the
// lognormal-jump sub-step U <- U + lambda dt (G U) at the end of every step.  lambda / mu / sigma: the shared jump law; lambda_i /
// mu_i / sigma_i: one value per instance, or empty = the shared value.  shared_grid: the caller's promise that every instance has
// instance 0's s-grid (checked by the library): with a shared (mu, sigma) one matrix serves the batch.  workspace.U is the caller's
// initial condition and receives the field.  compute_jacobian_bates keeps the five columns (the jump parameters are inputs);
// compute_jacobian_bates_jumps has eight.
struct Jumps {
    double lambda = 0.0, mu = 0.0, sigma = 0.1;
    std::vector<double> lambda_i, mu_i, sigma_i;
    bool shared_grid = false;
    hadi_jumps view(int num_strikes) const {
        for (const std::vector<double> *a : {&lambda_i, &mu_i, &sigma_i})
            if (!a->empty() && a->size() != (size_t)num_strikes) throw std::runtime_error("a jump array is not [num_strikes]");
        return hadi_jumps{lambda, mu, sigma, lambda_i.empty() ? nullptr : lambda_i.data(), mu_i.empty() ? nullptr : mu_i.data(),
                          sigma_i.empty() ? nullptr : sigma_i.data(), shared_grid ? 1 : 0};
    }
};
inline void bates_timestepping(Handle &h, int m1, int m2, int N, double delta_t, double theta, double r_d, double r_f, double rho,
                               double sigma, double kappa, double eta, int num_strikes, const GridViews &deviceGrids,
                               DO_Workspace &workspace, const Jumps &jumps, int variant = HADI_EU, const Dividends *div = nullptr,
                               const PutStrikes *put = nullptr) {
    const hadi_jumps j = jumps.view(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_bates_timestepping(h.ctx, &p, &j));
}
// ... with the v-grid rebuilt for V_0 and the price pick, as compute_base_prices does
inline void compute_base_prices_bates(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                      double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N,
                                      double theta, double delta_t, int num_strikes, const GridViews &deviceGrids,
                                      DO_Workspace &workspace, const Jumps &jumps, std::vector<double> &base_prices,
                                      int variant = HADI_EU, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_jumps j = jumps.view(num_strikes);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  workspace.U.data(), nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_bates(h.ctx, &p, S_0, V_0, &j, base_prices.data()));
}
// J: [num_strikes][5], base_prices: [num_strikes]; the six solves of an instance share its jump law and its matrix
inline void compute_jacobian_bates(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                   double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                   double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                   const Jumps &jumps, std::vector<double> &J, std::vector<double> &base_prices,
                                   double eps = 1e-6, int variant = HADI_EU, const Dividends *div = nullptr,
                                   const PutStrikes *put = nullptr) {
    const hadi_jumps j = jumps.view(num_strikes);
    J.resize((size_t)num_strikes * 5);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_bates(h.ctx, &p, S_0, V_0, eps, &j, J.data(), base_prices.data()));
}
// J: [num_strikes][8], columns kappa, eta, sigma, rho, V_0, lambda, mu_J, sigma_J -- the jump law among the parameters: nine solves
// per instance over three sets of matrices (hadi_compute_jacobian_bates_jumps); (lambda + eps) delta_t must not exceed 1
inline void compute_jacobian_bates_jumps(Handle &h, double S_0, double V_0, double /*T*/, double r_d, double r_f, double rho,
                                         double sigma, double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                         double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                         const Jumps &jumps, std::vector<double> &J, std::vector<double> &base_prices,
                                         double eps = 1e-6, int variant = HADI_EU, const Dividends *div = nullptr,
                                         const PutStrikes *put = nullptr) {
    const hadi_jumps j = jumps.view(num_strikes);
    J.resize((size_t)num_strikes * 8);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_bates_jumps(h.ctx, &p, S_0, V_0, eps, &j, J.data(), base_prices.data()));
}

// A Bates strike x maturity surface from one sweep (hadi_bates_sample_ladder and its two launchers; NOT in the reference): the
// sample calls above with the jump sub-step at the end of every step, in front of the snapshot.  The argument order is the sample
// functions' with `jumps` behind snap_steps.  out: [num_strikes][snap_steps.size()][n_samp].
inline void bates_sample_ladder(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma, double kappa,
                                double eta, int m1, int m2, int /*total_size*/, int N, double theta, double delta_t, int num_strikes,
                                const GridViews &deviceGrids, const DO_Workspace &workspace, const Samples &samples,
                                const std::vector<int> &snap_steps, const Jumps &jumps, std::vector<double> &out, int variant = HADI_EU,
                                const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    const hadi_jumps j = jumps.view(num_strikes);
    out.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_bates_sample_ladder(h.ctx, &p, V_0, &s, (int)snap_steps.size(), snap_steps.data(), &j, out.data()));
}
// ... with the v-grid rebuilt for V_0, as compute_base_prices does
inline void compute_base_prices_bates_samples(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                                              double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                              double delta_t, int num_strikes, const GridViews &deviceGrids,
                                              const DO_Workspace &workspace, const Samples &samples, const std::vector<int> &snap_steps,
                                              const Jumps &jumps, std::vector<double> &out, int variant = HADI_EU,
                                              const std::vector<double> *U_0 = nullptr, const Dividends *div = nullptr,
                                              const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    const hadi_jumps j = jumps.view(num_strikes);
    out.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  const_cast<double *>(workspace.U.data()), U_0 ? U_0->data() : nullptr, div, put);
    detail::check(h, hadi_compute_base_prices_bates_samples(h.ctx, &p, V_0, &s, (int)snap_steps.size(), snap_steps.data(), &j, out.data()));
}
// J: [num_strikes][snap_steps.size()][n_samp][n_par], base: [num_strikes][snap_steps.size()][n_samp]; n_par = 8 with jump_columns
// (kappa, eta, sigma, rho, V_0, lambda, mu_J, sigma_J), else 5
inline void compute_jacobian_bates_samples(Handle &h, double V_0, double /*T*/, double r_d, double r_f, double rho, double sigma,
                                           double kappa, double eta, int m1, int m2, int /*total_size*/, int N, double theta,
                                           double delta_t, int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                                           const Samples &samples, const std::vector<int> &snap_steps, const Jumps &jumps,
                                           bool jump_columns, std::vector<double> &J, std::vector<double> &base, double eps = 1e-6,
                                           int variant = HADI_EU, const Dividends *div = nullptr, const PutStrikes *put = nullptr) {
    const hadi_samples s = samples.view();
    const hadi_jumps j = jumps.view(num_strikes);
    const int n_par = jump_columns ? 8 : 5;
    J.resize((size_t)num_strikes * snap_steps.size() * s.n_samp * n_par);
    base.resize((size_t)num_strikes * snap_steps.size() * s.n_samp);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div, put);
    detail::check(h, hadi_compute_jacobian_bates_samples(h.ctx, &p, V_0, eps, &s, (int)snap_steps.size(), snap_steps.data(), &j, n_par,
                                                         J.data(), base.data()));
}

// jacobian_computation.cpp:204-364 and the three variants.  J: [num_strikes][5], columns kappa, eta, sigma, rho, v0.
inline void compute_jacobian(Handle &h, double S_0, double V_0, double, double r_d, double r_f, double rho, double sigma,
                             double kappa, double eta, int m1, int m2, int, int N, double theta, double delta_t,
                             int num_strikes, const GridViews &deviceGrids, const std::vector<double> &U_0,
                             std::vector<double> &J, std::vector<double> &base_prices, double eps = 1e-6,
                             int variant = HADI_EU, const Dividends *div = nullptr) {
    J.resize((size_t)num_strikes * 5);
    base_prices.resize(num_strikes);
    hadi_problem p = detail::make(variant, num_strikes, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                                  nullptr, U_0.data(), div);
    int rc;
    switch (variant) {
        case HADI_AM: rc = hadi_compute_jacobian_american(h.ctx, &p, S_0, V_0, eps, J.data(), base_prices.data()); break;
        case HADI_DIV: rc = hadi_compute_jacobian_dividends(h.ctx, &p, S_0, V_0, eps, J.data(), base_prices.data()); break;
        case HADI_AM_DIV: rc = hadi_compute_jacobian_american_dividends(h.ctx, &p, S_0, V_0, eps, J.data(), base_prices.data()); break;
        default: rc = hadi_compute_jacobian(h.ctx, &p, S_0, V_0, eps, J.data(), base_prices.data()); break;
    }
    detail::check(h, rc);
}
inline void compute_jacobian_american(Handle &h, double S_0, double V_0, double T, double r_d, double r_f, double rho,
                                      double sigma, double kappa, double eta, int m1, int m2, int ts, int N, double theta,
                                      double delta_t, int num_strikes, const GridViews &g, const std::vector<double> &U_0,
                                      std::vector<double> &J, std::vector<double> &base_prices, double eps = 1e-6) {
    compute_jacobian(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, ts, N, theta, delta_t, num_strikes, g, U_0, J,
                     base_prices, eps, HADI_AM, nullptr);
}
inline void compute_jacobian_dividends(Handle &h, double S_0, double V_0, double T, double r_d, double r_f, double rho,
                                       double sigma, double kappa, double eta, int m1, int m2, int ts, int N, double theta,
                                       double delta_t, int num_strikes, const GridViews &g, const std::vector<double> &U_0,
                                       const Dividends &div, std::vector<double> &J, std::vector<double> &base_prices,
                                       double eps = 1e-6) {
    compute_jacobian(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, ts, N, theta, delta_t, num_strikes, g, U_0, J,
                     base_prices, eps, HADI_DIV, &div);
}
inline void compute_jacobian_american_dividends(Handle &h, double S_0, double V_0, double T, double r_d, double r_f,
                                                double rho, double sigma, double kappa, double eta, int m1, int m2, int ts,
                                                int N, double theta, double delta_t, int num_strikes, const GridViews &g,
                                                const std::vector<double> &U_0, const Dividends &div, std::vector<double> &J,
                                                std::vector<double> &base_prices, double eps = 1e-6) {
    compute_jacobian(h, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, ts, N, theta, delta_t, num_strikes, g, U_0, J,
                     base_prices, eps, HADI_AM_DIV, &div);
}

// jacobian_computation.cpp:107-195
inline void compute_parameter_update_on_device(const std::vector<double> &J, const std::vector<double> &residuals,
                                               double lambda, std::vector<double> &delta) {
    delta.resize(5);
    if (hadi_compute_parameter_update((int)residuals.size(), J.data(), residuals.data(), lambda, delta.data()))
        throw std::runtime_error("hadi_compute_parameter_update failed");
}

// The LM normal equations for n_par = 1 .. HADI_LM_MAX_PAR parameters (hadi_lm_partials_n, hadi_lm_solve_n): J [n][n_par];
// partials = [J^T J row-major][J^T r][sum r^2], n_par^2 + n_par + 1 doubles -- what is all-reduced across ranks; delta [n_par].
inline void lm_partials_n(int n_par, const std::vector<double> &J, const std::vector<double> &residuals, std::vector<double> &partials) {
    if (n_par < 1 || J.size() != residuals.size() * (size_t)n_par) throw std::runtime_error("lm_partials_n: J is not [n][n_par]");
    partials.resize((size_t)n_par * n_par + n_par + 1);
    if (hadi_lm_partials_n((int)residuals.size(), n_par, J.data(), residuals.data(), partials.data()))
        throw std::runtime_error("hadi_lm_partials_n failed");
}
inline void lm_solve_n(int n_par, const std::vector<double> &partials, double lambda, std::vector<double> &delta) {
    if (n_par < 1 || partials.size() != (size_t)n_par * n_par + n_par + 1) throw std::runtime_error("lm_solve_n: partials are not of n_par parameters");
    delta.resize(n_par);
    if (hadi_lm_solve_n(n_par, partials.data(), lambda, delta.data())) throw std::runtime_error("hadi_lm_solve_n failed");
}

}  // namespace hadi_host
