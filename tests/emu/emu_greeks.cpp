// emu_greeks.cpp -- TEST-ONLY.  The wave emulator's driver of hadi_greeks_kernel (csrc/hadi_k_greeks.h): emu_driver.cpp
// (included whole) plus one entry point that builds the operator tables and packs a GIVEN field as the library does
// (hadi_setup_kernel, hadi_pack_kernel) and runs the Greeks kernel on it.  The field is the caller's -- the tests hand in the
// oracle's U_T and lambda_bar_T -- so the kernel is checked apart from any sweep.  Never shipped.
#include "emu_driver.cpp"

// Arrays natural layout [n][...].  par8 [n][8]: rho, sigma, kappa, eta, dt, N, strike, option type (0 call, 1 put), the rows
// fill_desc of hadi_api.hip builds.  LAM: lambda_bar at T for American variants, NULL otherwise.  greeks [n][8]; ladder
// [n][m1+1][8] or NULL; status [n] (0 ok, 1 S_0 off the s-grid, 2 V_0 off the v-grid).  The launch geometry is the library's
// (greeks_common; S_0 and V_0 reach it in its CallOut).  Returns 0, or 1 if the shape has no plan.
extern "C" int emu_greeks(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8,
                          const double *vec_s, const double *vec_v, const double *delta_s, const double *delta_v,
                          const double *U, const double *LAM, double S_0, double V_0, double *greeks, double *ladder,
                          int *status, int setup_threads, int *shape_out /*B, G, ntiles*/) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    const HadiLayout &L = pl.L;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dL(LAM ? st : 0);
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
    if (LAM) emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, LAM, dL.data()); });
    HadiGreeksArgs g;
    g.L = L; g.n_inst = n_inst; g.american = LAM ? 1 : 0;
    g.ntiles = L.B == 1 ? (m1 + HADI_GK_TILE) / HADI_GK_TILE : 1;
    g.span = L.B == 1 ? HADI_GK_TILE + 2 * HADI_GK_HALO : L.rowp;
    g.U = dU.data(); g.LAM = LAM ? dL.data() : nullptr;
    g.scoef = scoef.data(); g.b2row = b2row.data(); g.rowc = rowc.data(); g.ipar = ipar.data();
    g.vec_s = vec_s; g.vec_v = vec_v; g.delta_s = delta_s; g.delta_v = delta_v;
    g.S_0 = S_0; g.V_0 = V_0;
    g.greeks = greeks; g.ladder = ladder; g.status = status;
    if (shape_out) { shape_out[0] = L.B; shape_out[1] = L.G; shape_out[2] = g.ntiles; }
    emu::launch(n_inst * g.ntiles, HADI_GK_THREADS, [&]() { hadi_greeks_kernel(g); }, hadi_greeks_smem(g.span));
    return 0;
}
