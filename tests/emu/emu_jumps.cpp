// emu_jumps.cpp -- TEST-ONLY.  The wave emulator's driver of a Bates sweep: emu_small_sch.cpp (included whole, and with it
// emu_driver.cpp) plus entry points that build the tables and pack the initial field as the library does (hadi_setup_kernel,
// hadi_pack_kernel), build the dividend table, the weights a_k and the generators as stage_dividends / stage_jumps of hadi_api.hip
// do (hadi_jump_matrix_kernel into a zeroed buffer, hadi_jump_grid_check_kernel for a shared matrix), and run the streaming loop
// of enqueue_sub_batch with the copy of U and hadi_jump_kernel behind every step's last column pass.  Never shipped.
#include "emu_small_sch.cpp"

// Elements of the packed state of n_inst instances (0: no plan).
extern "C" long long emu_jumps_packed_size(int n_inst, int m1, int m2) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 0;
    return (long long)pl.L.inst_stride * n_inst;
}

// The natural-order generator [m1 + 1][m1 + 1] of one grid, as hadi_debug_jump_matrix returns it: hadi_jump_matrix_kernel into the
// zeroed operand-order buffer, then hadi_jump_matrix_unpack_kernel.  Returns 0, or 1 (no streaming layout).
extern "C" int emu_jump_matrix(int m1, const double *vec_s, double mu, double sigma, double *G_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, 8, 1, 8 * 256, &pl, g_tune, 8) || pl.row_seq) return 1;
    const HadiLayout &L = pl.L;
    const size_t ne = (size_t)(m1 + 1) * (m1 + 1);
    std::vector<double> G(hadi_jump_matrix_doubles(L), 0.0);
    const double ms[2] = {mu, sigma};
    emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, 1, vec_s, ms, G.data()); });
    emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_unpack_kernel(L, G.data(), G_out); });
    return 0;
}

// Arrays natural layout [n][...].  par8 [n][8]: rho, sigma, kappa, eta, dt, N, strike, put -- the rows fill_desc builds; N and dt
// may differ between instances.  The streaming kernels (the plan's own choice; emu_set_tuning "strip" pins it).  scheme: enum
// hadi_scheme.  U: the initial field (not modified).  lam, mu, sig [n], or lam NULL: no jump tables at all (the plain run).
// shared: one matrix for the batch, built on instance 0's grid with (mu[0], sig[0]); ipg: instances per block of hadi_jump_kernel
// (the library takes 1 unless the matrix is shared).  U_out [n][m].  P_out (or NULL) [emu_jumps_packed_size]: the packed state
// the sweep leaves; is_pad (or NULL), same size: 1 where the element is no node (a pad slot, a slot of a node beyond m1, an identity
// row).  stat_out (or NULL): the word of the shared-grid check.
// Returns 0, 1 (no plan), 2 (no such kernel), 3 (not admitted), 4 (device error word set).
extern "C" int emu_jumps(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8, const double *vec_s,
                         const double *vec_v, const double *delta_s, const double *delta_v, const double *U, int scheme, int ndiv,
                         const double *ddates, const double *damounts, const double *dpcts, const double *lam, const double *mu,
                         const double *sig, int shared, int ipg, double *U_out, double *P_out, unsigned char *is_pad, int *stat_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    if (hadi_no_strips(theta, r_d == r_f)) pl.use_strip = 0;
    const HadiLayout &L = pl.L;
    const bool dividend = ndiv > 0, cs = scheme != 0;
    if (scheme < 0 || scheme > 3 || (cs && dividend) || pl.row_seq || pl.col_seq || ipg < 1) return 3;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dY(st, 0.0), dUT(st), dV(cs ? st : 0), dR1(cs ? st : 0), dC2(cs ? st : 0);
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
    int Nmax = 0;
    bool uniform = true;
    for (int k = 0; k < n_inst; k++) {
        Nmax = std::max(Nmax, (int)par8[(size_t)k * 8 + 5]);
        uniform = uniform && par8[(size_t)k * 8 + 5] == par8[5] && par8[(size_t)k * 8 + 4] == par8[4];
    }
    const int flag_stride = uniform ? 0 : Nmax;
    std::vector<int> flags((size_t)(uniform ? 1 : n_inst) * Nmax, -1);
    std::vector<char> div_step(Nmax + 1, 0);
    if (dividend)
        for (int k = 0; k < (uniform ? 1 : n_inst); k++) {
            int *f = flags.data() + (size_t)k * Nmax;
            hadi_dividend_steps((int)par8[(size_t)k * 8 + 5], par8[(size_t)k * 8 + 4], ndiv, ddates, f, Nmax);
            for (int q = 0; q < Nmax; q++)
                if (f[q] >= 0) div_step[q + 1] = 1;
        }
    // the weights and the matrices, as apply_extras and stage_jumps build them
    std::vector<double> avec(n_inst, 0.0), musig, G;
    bool jumps = false;
    for (int k = 0; lam && k < n_inst; k++) {
        avec[k] = lam[k] * par8[(size_t)k * 8 + 4];
        jumps = jumps || avec[k] != 0.0;
    }
    const int n_mat = shared ? 1 : n_inst;
    int stat = 0;
    if (jumps) {
        for (int q = 0; q < n_mat; q++) { musig.push_back(mu[q]); musig.push_back(sig[q]); }
        G.assign((size_t)n_mat * hadi_jump_matrix_doubles(L), 0.0);
        const size_t ne = (size_t)n_mat * (m1 + 1) * (m1 + 1);
        emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, n_mat, vec_s, musig.data(), G.data()); });
        if (shared)
            emu::launch((unsigned)(((size_t)n_inst * (m1 + 1) + 255) / 256), 256,
                        [&]() { hadi_jump_grid_check_kernel(m1 + 1, n_inst, vec_s, &stat); });
    }
    if (stat_out) *stat_out = stat;
    HadiSweepArgs a{};
    a.U = dU.data(); a.Y = dY.data();
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw;
    a.bgroups = pl.bgroups; a.tile_il = g_tile_il; a.pos_m1 = pl.pos_m1; a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = &g_err; a.debug = g_debug;
    a.R1 = cs ? dR1.data() : nullptr; a.C2 = cs ? dC2.data() : nullptr;
    const bool pair_tab = hadi_pair_table(pl, cs) && pl.use_strip;
    std::vector<double> dRS(pair_tab ? (size_t)n_inst * L.nrows * 128 : 0, std::nan(""));
    a.rs_tab = pair_tab ? dRS.data() : nullptr;
    HadiSweepArgs av = a;
    if (cs) av.U = dV.data();
    if (pair_tab && run_pass(hadi_select_pair_table(pl), a, 1)) return 2;
    for (int n = 1; n <= Nmax; n++) {
        if (dividend && div_step[n]) {
            dUT = dU;
            emu::launch(8, 64, [&]() {
                hadi_dividend_kernel(L, n_inst, ipar.data(), vec_s, dUT.data(), dU.data(), flags.data(), flag_stride, n, damounts, dpcts);
            });
        }
        const HadiPassCtx pc{pl, n_inst, false, false, false, false, scheme, g_cs_strips, g_col_prefetch};
        const HadiSel col = hadi_select_col_pass(pc);
        for (int mode = cs ? 1 : 0; mode <= (cs ? 2 : 0); mode++)
            if (run_pass(hadi_select_row_pass(pc, mode), mode == 2 ? av : a, n) || run_pass(col, mode == 1 ? av : a, n)) return 2;
        if (jumps) {  // U_temp <- U, then the sub-step out of place
            dUT = dU;
            emu::launch(hadi_jump_grid(L, n_inst, ipg), HADI_JUMP_THREADS, [&]() {
                hadi_jump_kernel(L, n_inst, ipg, 0, n_inst, dUT.data(), dU.data(), G.data(),
                                 shared ? 0ll : (long long)hadi_jump_matrix_doubles(L), avec.data(), ipar.data(), n);
            }, hadi_jump_smem(L));
        }
    }
    emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U_out); });
    if (P_out) std::copy(dU.begin(), dU.end(), P_out);
    if (is_pad)
        for (size_t e = 0; e < st; e++) {
            const size_t r = e % (size_t)L.inst_stride;
            const int i = hadi_slot_to_i(L, (int)(r % L.rowp));
            is_pad[e] = (i < 0 || i > L.m1 || (int)(r / L.rowp) >= L.nrows) ? 1 : 0;
        }
    return g_err ? 4 : 0;
}

// emu_route (emu_driver.cpp) with the one input a Bates call adds: some weight a_k is not zero.  o[16]: emu_route's 15 words and
// HadiRoute::jumps.
extern "C" int emu_route_jumps(const int *in, double theta, const char *tuning, int jumps, long long *o, int *subs, int max_subs,
                               char *desc, int cap) {
    HadiRouteIn ri;
    ri.cu_count = in[0]; ri.n = in[1]; ri.m1 = in[2]; ri.m2 = in[3]; ri.variant = in[4]; ri.scheme = in[5]; ri.prec = in[6];
    ri.theta = theta; ri.rates_equal = in[7] != 0; ri.debug = in[8]; ri.profiling = in[9] != 0; ri.n_snap = in[10];
    ri.dividends = in[11] != 0; ri.uniform_steps = in[12] != 0; ri.team_failed = in[13] != 0;
    ri.jumps = jumps != 0;
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
    for (int k = 0; k < (int)r.bp.subs.size() && k < max_subs; k++) {
        const int s4[4] = {r.bp.subs[k].off, r.bp.subs[k].cnt, r.bp.subs[k].lane, r.resident[k]};
        std::copy(s4, s4 + 4, subs + 4 * k);
    }
    std::snprintf(desc, cap, "%s", hadi_describe_route(r, ri, in[14] != 0, in[15]).c_str());
    return 0;
}
