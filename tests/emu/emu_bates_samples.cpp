// emu_bates_samples.cpp -- TEST-ONLY.  The wave emulator's driver of a sampled Bates ladder (hadi_bates_sample_ladder and its
// launchers): emu_jumps.cpp (included whole, and with it emu_small_sch.cpp and emu_driver.cpp) plus one entry point that builds the
// tables, packs the initial field, locates the samples and builds the weights and the generators as the library does
// (hadi_setup_kernel, hadi_pack_kernel, hadi_sample_locate_kernel, hadi_jump_matrix_kernel, hadi_jump_grid_check_kernel), and then
// runs either hadi_small_jump_kernel -- the whole time loop with the jump stage -- or the streaming loop of enqueue_sub_batch: the
// copy of U, hadi_jump_kernel / hadi_jump_sel_kernel and, on snapshot steps, hadi_sample_kernel.  Never shipped.
#include "emu_jumps.cpp"

// The batch is `n_inst` instances, the rows of `n0` source instances repeated group by group (n_inst = n0: a plain batch; 6 n0 or 9 n0:
// a Jacobian's).  par8, vec_s, vec_v, delta_s, delta_v hold all n_inst rows; U [n0][m]: the initial field of the source instances.
// lam [n_inst]: every instance's intensity (the caller has bumped the lambda group).  musig [n_mat][2]: the matrices' (mu, sigma), matrix
// q built on row q of vec_s, as stage_jumps builds them; sets: 1, or 3 = the three matrix sets of nine groups, n_mat = sets * per, per 1
// (shared: one matrix per set, the grid check runs) or n0.  Instance k uses matrix (set of group k / n0) * per + (per > 1 ? k % n0 : 0).
// how: 0 the streaming loop, 4 / 8 hadi_small_jump_kernel with that many wavefronts per instance.  V0_i [n_inst] or NULL (then V_0).
// spots / scales [rows][n_samp], rows 1 or n0 (scales may be NULL).  out [n_inst][n_snap][n_samp], flags [n_inst][n_samp].  P_out (or
// NULL) [emu_jumps_packed_size]: the packed state the sweep leaves; is_pad (or NULL), same size: 1 where the element is no node.
// stat_out (or NULL): the word of the shared-grid check.
// Returns 0, 1 (no plan), 2 (no such kernel), 3 (not admitted), 4 (device error word set).
extern "C" int emu_bates_samples(int n_inst, int n0, int m1, int m2, double theta, double r_d, double r_f, const double *par8,
                                 const double *vec_s, const double *vec_v, const double *delta_s, const double *delta_v, const double *U,
                                 int ndiv, const double *ddates, const double *damounts, const double *dpcts, const double *lam,
                                 const double *musig, int n_mat, int sets, int shared, int how, double V_0, const double *V0_i, int n_samp,
                                 const double *spots, const double *scales, int rows, int n_snap, const int *snap_steps, double *out,
                                 int *flags, double *P_out, unsigned char *is_pad, int *stat_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    if (hadi_no_strips(theta, r_d == r_f)) pl.use_strip = 0;
    const HadiLayout &L = pl.L;
    const bool dividend = ndiv > 0;
    if (pl.row_seq || pl.col_seq || n_samp < 1 || n_snap < 1 || (rows != 1 && rows != n0) || n_inst % n0 || (sets != 1 && sets != 3)) return 3;
    if (lam && (n_mat % sets || (n_mat / sets != 1 && n_mat / sets != n0) || (shared && n_mat != sets) ||
                (sets == 3 && n_inst != HADI_JUMP_GROUPS * n0)))
        return 3;
    if (how != 0 && how != 4 && how != 8) return 3;
    if (how && !(pl.smem_small_eu > 0)) return 3;
    const int per = n_mat / sets;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dY(st, 0.0), dUT(st);
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
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n0, U, dU.data()); });
    // a ladder shares the step indices; delta_t may differ
    const int N = (int)par8[5];
    bool uniform = true;
    for (int k = 0; k < n_inst; k++) {
        if ((int)par8[(size_t)k * 8 + 5] != N) return 3;
        uniform = uniform && par8[(size_t)k * 8 + 4] == par8[4];
    }
    for (int q = 0; q < n_snap; q++)
        if (snap_steps[q] < 1 || snap_steps[q] > N || (q && snap_steps[q] <= snap_steps[q - 1])) return 3;
    const int flag_stride = uniform ? 0 : N;
    std::vector<int> dflags((size_t)(uniform ? 1 : n_inst) * N, -1);
    std::vector<char> div_step(N + 1, 0);
    if (dividend)
        for (int k = 0; k < (uniform ? 1 : n_inst); k++) {
            int *f = dflags.data() + (size_t)k * N;
            hadi_dividend_steps(N, par8[(size_t)k * 8 + 4], ndiv, ddates, f, N);
            for (int q = 0; q < N; q++)
                if (f[q] >= 0) div_step[q + 1] = 1;
        }
    // the samples' lists and tap records
    const size_t ns = (size_t)n_inst * n_samp;
    std::vector<double> in(2 * ns);
    for (int k = 0; k < n_inst; k++)
        for (int q = 0; q < n_samp; q++) {
            const size_t src = (size_t)(rows > 1 ? k % n0 : 0) * n_samp + q;
            in[(size_t)k * n_samp + q] = spots[src];
            in[ns + (size_t)k * n_samp + q] = scales ? scales[src] : 1.0;
        }
    std::vector<HadiTap> taps(ns);
    emu::launch((int)((ns + 255) / 256), 256, [&]() {
        hadi_sample_locate_kernel(L, n_inst, n_samp, vec_s, vec_v, V0_i, V_0, in.data(), in.data() + ns, taps.data(), flags);
    });
    // the weights and the matrices
    std::vector<double> avec(n_inst, 0.0);
    bool jumps = false;
    for (int k = 0; lam && k < n_inst; k++) {
        avec[k] = lam[k] * par8[(size_t)k * 8 + 4];
        jumps = jumps || avec[k] != 0.0;
    }
    std::vector<double> G;
    std::vector<int> mat(n_inst, 0);
    int stat = 0;
    if (jumps) {
        G.assign((size_t)n_mat * hadi_jump_matrix_doubles(L), 0.0);
        const size_t ne = (size_t)n_mat * (m1 + 1) * (m1 + 1);
        emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, n_mat, vec_s, musig, G.data()); });
        if (shared)
            emu::launch((unsigned)(((size_t)n_inst * (m1 + 1) + 255) / 256), 256,
                        [&]() { hadi_jump_grid_check_kernel(m1 + 1, n_inst, vec_s, &stat); });
        for (int k = 0; k < n_inst; k++) mat[k] = (sets > 1 ? hadi_jump_set(k / n0) : 0) * per + (per > 1 ? k % n0 : 0);
    }
    if (stat_out) *stat_out = stat;
    HadiSweepArgs a{};
    a.U = dU.data(); a.Y = dY.data();
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw;
    a.bgroups = pl.bgroups; a.tile_il = g_tile_il; a.pos_m1 = pl.pos_m1; a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = &g_err; a.debug = g_debug;
    if (how) {  // the whole time loop in one launch
        std::vector<int> node(n_inst, -1);
        std::vector<double> snap_out((size_t)n_inst * n_snap, 0.0);  // (the single node's output: must stay untouched)
        HadiSmallArgs sm;
        sm.div_flag = dividend ? dflags.data() : nullptr; sm.flag_stride = flag_stride; sm.div_amounts = damounts; sm.div_pcts = dpcts;
        sm.vec_s = vec_s; sm.Nmax = N; sm.order = nullptr;
        sm.snap_steps = snap_steps; sm.n_snap = n_snap; sm.snap_node = node.data(); sm.snap_out = snap_out.data();
        sm.taps = taps.data(); sm.n_samp = n_samp; sm.samp_out = out;
        if (jumps) {
            sm.jmp_G = G.data(); sm.jmp_a = avec.data(); sm.jmp_mat = mat.data(); sm.jmp_stride = (long long)hadi_jump_matrix_doubles(L);
        }
        const HadiLoopFn fn = hadi_small_jump_fn(L.B, how);
        if (!fn) return 2;
        emu::launch(n_inst, 64 * how, [&]() { fn(a, sm); }, pl.smem_small_eu);
        for (double x : snap_out)
            if (x != 0.0) return 5;
    } else {  // the streaming loop: passes, copy, jump kernel, sample kernel
        const bool pair_tab = hadi_pair_table(pl, false) && pl.use_strip;
        std::vector<double> dRS(pair_tab ? (size_t)n_inst * L.nrows * 128 : 0, std::nan(""));
        a.rs_tab = pair_tab ? dRS.data() : nullptr;
        if (pair_tab && run_pass(hadi_select_pair_table(pl), a, 1)) return 2;
        int q = 0;
        for (int n = 1; n <= N; n++) {
            if (dividend && div_step[n]) {
                dUT = dU;
                emu::launch(8, 64, [&]() {
                    hadi_dividend_kernel(L, n_inst, ipar.data(), vec_s, dUT.data(), dU.data(), dflags.data(), flag_stride, n, damounts, dpcts);
                });
            }
            const HadiPassCtx pc{pl, n_inst, false, false, false, false, 0, g_cs_strips, g_col_prefetch};
            if (run_pass(hadi_select_row_pass(pc, 0), a, n) || run_pass(hadi_select_col_pass(pc), a, n)) return 2;
            if (jumps) {
                dUT = dU;
                const long long gs = (long long)hadi_jump_matrix_doubles(L);
                if (sets > 1) {
                    const HadiJumpSel js{0, n0, per, 0, 1};
                    emu::launch(hadi_jump_sel_grid(L, js, n_inst), HADI_JUMP_THREADS, [&]() {
                        hadi_jump_sel_kernel(L, n_inst, js, dUT.data(), dU.data(), G.data(), gs, avec.data(), ipar.data(), n);
                    }, hadi_jump_smem(L));
                } else {
                    emu::launch(hadi_jump_grid(L, n_inst, 1), HADI_JUMP_THREADS, [&]() {
                        hadi_jump_kernel(L, n_inst, 1, 0, n0, dUT.data(), dU.data(), G.data(), per > 1 ? gs : 0ll, avec.data(), ipar.data(), n);
                    }, hadi_jump_smem(L));
                }
            }
            if (q < n_snap && n == snap_steps[q]) {
                emu::launch((int)((ns + 255) / 256), 256, [&]() { hadi_sample_kernel(L, n_inst, dU.data(), taps.data(), out, n_snap, n_samp, q); });
                q++;
            }
        }
    }
    if (P_out) std::copy(dU.begin(), dU.end(), P_out);
    if (is_pad)
        for (size_t e = 0; e < st; e++) {
            const size_t r = e % (size_t)L.inst_stride;
            const int i = hadi_slot_to_i(L, (int)(r % L.rowp));
            is_pad[e] = (i < 0 || i > L.m1 || (int)(r / L.rowp) >= L.nrows) ? 1 : 0;
        }
    return g_err ? 4 : 0;
}

// Layout words of the plan of a shape, for the tests' own assertions: B, rowp, nrows, the LDS bytes of the block kernel (0: not admitted).
extern "C" int emu_bates_samples_layout(int m1, int m2, int n_inst, long long *o4) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    o4[0] = pl.L.B; o4[1] = pl.L.rowp; o4[2] = pl.L.nrows; o4[3] = (long long)pl.smem_small_eu;
    return 0;
}

// emu_route_jumps (emu_jumps.cpp) with the second input of a sampled Bates ladder: n_samp samples per instance and snapshot (in[10] is
// n_snap, as there).  o[16]: emu_route's 15 words and HadiRoute::jumps.
extern "C" int emu_route_bates_samples(const int *in, double theta, const char *tuning, int jumps, int n_samp, long long *o, char *desc,
                                       int cap) {
    HadiRouteIn ri;
    ri.cu_count = in[0]; ri.n = in[1]; ri.m1 = in[2]; ri.m2 = in[3]; ri.variant = in[4]; ri.scheme = in[5]; ri.prec = in[6];
    ri.theta = theta; ri.rates_equal = in[7] != 0; ri.debug = in[8]; ri.profiling = in[9] != 0; ri.n_snap = in[10];
    ri.dividends = in[11] != 0; ri.uniform_steps = in[12] != 0; ri.team_failed = in[13] != 0;
    ri.jumps = jumps != 0; ri.n_samp = n_samp;
    for (std::string rest(tuning ? tuning : ""); !rest.empty();) {
        const size_t comma = rest.find(','), eq = rest.find('=');
        if (eq == std::string::npos || eq > comma) return 2;
        const HadiTuneKey *e = hadi_tuning_key(rest.substr(0, eq).c_str());
        if (!e || hadi_tuning_set(ri.t, *e, std::atoi(rest.c_str() + eq + 1))) return 2;
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
    }
    const HadiRoute r = hadi_route(ri);
    o[0] = r.status;
    if (r.status) return 1;
    const long long v[16] = {r.status, r.kind, r.small_waves, (long long)r.bp.subs.size(), r.bp.two_streams, r.bp.fork_before, r.n_resident(),
                             r.read_payoff_shape, r.pair_tab, r.need_lam_u0, r.need_ut, r.need_f32, r.need_v_r1_c2, r.need_r1, r.graphable,
                             r.jumps};
    std::copy(v, v + 16, o);
    std::snprintf(desc, cap, "%s", hadi_describe_route(r, ri, false, HADI_TEAM_NOT_RUN).c_str());
    return 0;
}
