// emu_resident.cpp -- TEST-ONLY.  The wave emulator's driver of the resident sweep (hadi_sweep_resident, csrc/hadi_k_resident.h):
// emu_driver.cpp (included whole: its kernels, tuning hooks and emu_solve for the streaming path) plus one entry point that sets
// up a batch as emu_solve does and runs its whole time loop in ONE launch of the resident kernel.  Never shipped.
#include "emu_driver.cpp"

// European Douglas sweep.  Arrays natural layout [n][...]; N_i / dt_i: per-instance step grids (NULL: N and dt for every
// instance; the launch runs to the largest N_i and every block stops at its own).  strike / put: per-instance strikes and the
// option type (put != 0: put boundary data K e^{-r_d t}; they fill par8[6] and par8[7] as fill_desc of hadi_api.hip does).  The strip geometry is forced to ONE block
// per instance (tuning "strip" = 1, "strip_blocks" = 1 on top of the emulator's tuning), whatever the batch size: the
// library's selection rules are tested on the GPU.  Returns 0, 1 (no plan), 3 (the shape is not eligible) or 4 (device error
// word set).
extern "C" int emu_solve_resident(int n_inst, int m1, int m2, int N, double dt, double theta, double r_d, double r_f,
                                  const double *par /*[n][4] rho sigma kappa eta*/, const double *vec_s, const double *vec_v,
                                  const double *delta_s, const double *delta_v, double *U, int setup_threads, const int *N_i,
                                  const double *dt_i, int *P_out, const double *strike /*[n], NULL with put = 0*/, int put) {
    HadiTuning tu = g_tune;
    tu.strip = 1;
    tu.strip_blocks = 1;
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, tu, 8)) return 1;
    const HadiLayout &L = pl.L;
    if (P_out) *P_out = L.P;
    if (!hadi_resident_grid(pl, theta, r_d == r_f) || !hadi_resident_plan(pl)) return 3;
    if ((N_i || dt_i) && (!N_i || !dt_i)) return 3;
    if (put && !strike) return 3;
    int Nmax = N;
    if (N_i) {
        Nmax = 0;
        for (int k = 0; k < n_inst; k++) Nmax = N_i[k] > Nmax ? N_i[k] : Nmax;
    }
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dY(st, 0.0);
    std::vector<double> scoef(pl.n_scoef * n_inst), b2row(pl.n_b2row * n_inst), rowc(pl.n_rowc * n_inst),
        a2i(pl.n_a2i * n_inst), pb(pl.n_pb * n_inst), rinv(pl.n_rinv * n_inst), rwork(pl.n_rwork * n_inst);
    std::vector<HadiInstPar> ipar(n_inst);
    std::vector<double> par8((size_t)n_inst * 8, 0.0);
    for (int k = 0; k < n_inst; k++) {
        for (int z = 0; z < 4; z++) par8[(size_t)k * 8 + z] = par[(size_t)k * 4 + z];
        par8[(size_t)k * 8 + 4] = dt_i ? dt_i[k] : dt;
        par8[(size_t)k * 8 + 5] = (double)(N_i ? N_i[k] : N);
        par8[(size_t)k * 8 + 6] = put ? strike[k] : 0.0;
        par8[(size_t)k * 8 + 7] = put ? 1.0 : 0.0;
    }
    HadiSetupArgs s;
    s.L = L; s.n_inst = n_inst;
    s.vec_s = vec_s; s.vec_v = vec_v; s.delta_s = delta_s; s.delta_v = delta_v;
    s.par = par8.data(); s.r_d = r_d; s.r_f = r_f; s.theta = theta;
    s.scoef = scoef.data(); s.b2row = b2row.data(); s.rowc = rowc.data(); s.a2i = a2i.data();
    s.pb = pb.data(); s.rinv = rinv.data(); s.rwork = rwork.data(); s.ipar = ipar.data();
    emu::launch(n_inst, setup_threads, [&]() { hadi_setup_kernel(s); });
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U, dU.data()); });
    HadiSweepArgs a;
    std::memset(&a, 0, sizeof a);
    a.U = dU.data(); a.Y = dY.data(); a.LAM = nullptr; a.U0 = nullptr; a.pay_mis = nullptr;
    a.R1 = nullptr; a.C2 = nullptr; a.rs_tab = nullptr;
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw;
    a.bgroups = pl.bgroups; a.tile_il = g_tile_il; a.american = 0; a.pos_m1 = pl.pos_m1; a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = &g_err; a.debug = 0;
    if (run_pass(hadi_select_resident(pl), a, Nmax)) return 3;
    emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U); });
    return g_err ? 4 : 0;
}
