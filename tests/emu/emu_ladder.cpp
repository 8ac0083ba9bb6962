// emu_ladder.cpp -- TEST-ONLY.  The wave emulator's driver of the maturity ladder of the four whole-loop kernels (hadi_small_kernel,
// hadi_small_seq_kernel, hadi_small_seq2_kernel, hadi_small_sch_kernel): emu_driver.cpp (included whole) plus one entry point
// that builds the tables, packs the initial field and locates the price node as the library does (hadi_setup_kernel,
// hadi_pack_kernel, hadi_locate_kernel), runs the kernel's whole time loop with the snapshot list and returns the snapshots.
// Never shipped.
#include "emu_driver.cpp"

// Arrays natural layout [n][...].  par8 [n][8]: rho, sigma, kappa, eta, dt, N, strike, put -- the rows fill_desc of hadi_api.hip
// builds (one N for the whole batch: a ladder shares the step indices).  kind: 0 / 1 hadi_small_kernel with 4 / 8 wavefronts,
// 2 hadi_small_seq_kernel, 3 hadi_small_seq2_kernel, 4 hadi_small_sch_kernel (scheme: enum hadi_scheme 1 .. 3; else 0).
// variant: bit 0 American (kinds 0 / 1 only), bit 1 dividends.  U: the initial field (not modified); U0: the payoff or NULL.
// out [n][n_snap]: the snapshots; U_out [n][m] or NULL: the field after the last step; status [n]: the locate step's words.
// Returns 0, 1 (no plan), 2 (no such kernel), 3 (not admitted).
extern "C" int emu_ladder(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8,
                          const double *vec_s, const double *vec_v, const double *delta_s, const double *delta_v,
                          const double *U, const double *U0, int kind, int variant, int scheme, int ndiv, const double *ddates,
                          const double *damounts, const double *dpcts, double S_0, double V_0, int n_snap, const int *snap_steps,
                          double *out, double *U_out, int *status) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    const HadiLayout &L = pl.L;
    const int american = variant & 1, dividend = (variant >> 1) & 1;
    if (kind < 0 || kind > 4) return 3;
    if (american && kind > 1) return 3;
    if (kind == 4 && (scheme < 1 || scheme > 3 || !hadi_small_sch_admits(L) || american || dividend)) return 3;
    if (kind < 4 && (scheme != 0 || !((american ? pl.smem_small_am : pl.smem_small_eu) > 0))) return 3;
    if (kind == 3 && L.nrows > 32) return 3;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dLAM(american ? st : 0, 0.0), dU0(american ? st : 0);
    std::vector<double> scoef(pl.n_scoef * n_inst), b2row(pl.n_b2row * n_inst), rowc(pl.n_rowc * n_inst),
        a2i(pl.n_a2i * n_inst), pb(pl.n_pb * n_inst), rinv(pl.n_rinv * n_inst), rwork(pl.n_rwork * n_inst);
    std::vector<HadiInstPar> ipar(n_inst);
    HadiSetupArgs s;
    s.L = L; s.n_inst = n_inst;
    s.vec_s = vec_s; s.vec_v = vec_v; s.delta_s = delta_s; s.delta_v = delta_v;
    s.par = par8; s.r_d = r_d; s.r_f = r_f; s.theta = theta;
    s.scoef = scoef.data(); s.b2row = b2row.data(); s.rowc = rowc.data(); s.a2i = a2i.data();
    s.pb = pb.data(); s.rinv = rinv.data(); s.rwork = rwork.data(); s.ipar = ipar.data();
    emu::launch(n_inst, 64, [&]() { hadi_setup_kernel(s); });
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U, dU.data()); });
    if (american) emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U0 ? U0 : U, dU0.data()); });
    std::vector<int> node(n_inst, -7);
    emu::launch((n_inst + 63) / 64, 64, [&]() {
        hadi_locate_kernel(L, n_inst, vec_s, vec_v, S_0, (const double *)nullptr, V_0, node.data(), status);
    });
    HadiSweepArgs a{};
    a.U = dU.data(); a.LAM = american ? dLAM.data() : nullptr; a.U0 = american ? dU0.data() : nullptr;
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.pos_m1 = pl.pos_m1; a.american = american;
    a.err = &g_err; a.debug = g_debug;
    const int N = (int)par8[5];
    for (int k = 0; k < n_inst; k++)
        if ((int)par8[(size_t)k * 8 + 5] != N) return 3;
    // dividend table: one row per instance (each dates the schedule on its own dt), as the library does for delta_t_i batches
    std::vector<int> flags((size_t)n_inst * N, -1);
    if (dividend)
        for (int k = 0; k < n_inst; k++) hadi_dividend_steps(N, par8[(size_t)k * 8 + 4], ndiv, ddates, flags.data() + (size_t)k * N, N);
    HadiSmallArgs sm;
    sm.div_flag = dividend ? flags.data() : nullptr; sm.flag_stride = N; sm.div_amounts = damounts; sm.div_pcts = dpcts;
    sm.vec_s = vec_s; sm.Nmax = N; sm.order = nullptr;
    sm.snap_steps = snap_steps; sm.n_snap = n_snap; sm.snap_node = node.data(); sm.snap_out = out;
    if (kind == 4) {
        const HadiLoopFn fn = hadi_small_sch_fn(L.B, scheme == 2 ? HADI_SCH_MCS : scheme == 3 ? HADI_SCH_HV : HADI_SCH_CS);
        if (!fn) return 2;
        emu::launch(n_inst, 64, [&]() { fn(a, sm); }, hadi_small_sch_smem(L));
    } else {
        const HadiSel sel = hadi_select_small(pl, n_inst, kind == 3 ? 2 : kind == 2 ? 1 : 0, kind == 1 ? 8 : 4, american != 0);
        if (!sel.k) return 2;
        emu::launch(sel.grid, sel.block, [&]() { sel.k->loop(a, sm); }, sel.smem);
    }
    if (U_out) emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U_out); });
    return g_err ? 4 : 0;
}
