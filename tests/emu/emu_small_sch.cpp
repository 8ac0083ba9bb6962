// emu_small_sch.cpp -- TEST-ONLY.  The wave emulator's driver of hadi_small_sch_kernel (csrc/hadi_k_small_sch.h): emu_driver.cpp
// (included whole) plus one entry point that builds the operator tables and packs the initial field as the library does
// (hadi_setup_kernel, hadi_pack_kernel), runs the kernel's whole time loop and unpacks the result.  Never shipped.
#include "emu_driver.cpp"

// Arrays natural layout [n][...].  par8 [n][8]: rho, sigma, kappa, eta, dt, N, 0, 0 (call boundary data), the rows fill_desc
// of hadi_api.hip builds.  scheme: enum hadi_scheme (1 Craig-Sneyd, 2 Modified Craig-Sneyd, 3 Hundsdorfer-Verwer).  The time
// loop runs to the largest N_i with the instances dispatched longest first, as in the library.  U: initial field in, U_T out.
// lds_bytes (may be NULL) receives the kernel's dynamic LDS.  Returns 0, 1 (no plan), 2 (no such kernel), 3 (grid or scheme
// not admitted).
extern "C" int emu_small_sch(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8,
                             const double *vec_s, const double *vec_v, const double *delta_s, const double *delta_v,
                             double *U, int scheme, int setup_threads, long long *lds_bytes) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    const HadiLayout &L = pl.L;
    if (scheme < 1 || scheme > 3 || !hadi_small_sch_admits(L)) return 3;
    if (scheme >= 2 && !(theta > 0.0)) return 3;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st);
    std::vector<double> scoef(pl.n_scoef * n_inst), b2row(pl.n_b2row * n_inst), rowc(pl.n_rowc * n_inst),
        a2i(pl.n_a2i * n_inst), pb(pl.n_pb * n_inst), rinv(pl.n_rinv * n_inst), rwork(pl.n_rwork * n_inst);
    std::vector<HadiInstPar> ipar(n_inst);
    HadiSetupArgs s;
    s.L = L; s.n_inst = n_inst;
    s.vec_s = vec_s; s.vec_v = vec_v; s.delta_s = delta_s; s.delta_v = delta_v;
    s.par = par8; s.r_d = r_d; s.r_f = r_f; s.theta = theta;
    s.scoef = scoef.data(); s.b2row = b2row.data(); s.rowc = rowc.data(); s.a2i = a2i.data();
    s.pb = pb.data(); s.rinv = rinv.data(); s.rwork = rwork.data(); s.ipar = ipar.data();
    emu::launch(n_inst, setup_threads, [&]() { hadi_setup_kernel(s); });
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U, dU.data()); });
    HadiSweepArgs a{};
    a.U = dU.data();
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.pos_m1 = pl.pos_m1;
    a.err = &g_err; a.debug = g_debug;
    int Nmax = 0;
    std::vector<int> order(n_inst);
    for (int k = 0; k < n_inst; k++) {
        order[k] = k;
        Nmax = std::max(Nmax, (int)par8[(size_t)k * 8 + 5]);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return par8[(size_t)x * 8 + 5] > par8[(size_t)y * 8 + 5]; });
    HadiSmallArgs sm;
    sm.div_flag = nullptr; sm.flag_stride = 0; sm.div_amounts = nullptr; sm.div_pcts = nullptr;
    sm.vec_s = vec_s; sm.Nmax = Nmax; sm.order = order.data();
    const HadiLoopFn fn = hadi_small_sch_fn(L.B, scheme == 2 ? HADI_SCH_MCS : scheme == 3 ? HADI_SCH_HV : HADI_SCH_CS);
    if (!fn) return 2;
    const size_t smem = hadi_small_sch_smem(L);
    if (lds_bytes) *lds_bytes = (long long)smem;
    emu::launch(n_inst, 64, [&]() { fn(a, sm); }, smem);
    emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U); });
    return g_err ? 4 : 0;
}
