// emu_cliquet.cpp -- TEST-ONLY.  The wave emulator's driver of a sweep with strike fixings (forward-start options, cliquets):
// emu_small_sch.cpp (included whole, and with it emu_driver.cpp: the two plain drivers the n_fix = 0 runs are compared with,
// emu_solve and emu_small_sch) plus one entry point that builds the tables and packs the initial field and the payoff as the library
// does (hadi_setup_kernel, hadi_pack_kernel), builds the dividend, fixing and weight tables as stage_dividends / stage_step_flags /
// stage_cliquet of hadi_api.hip do, locates the reference nodes (hadi_fixing_locate_kernel), and runs either a whole-loop kernel
// (the event inside its time loop) or the streaming loop of enqueue_sub_batch with hadi_fixing_gather_kernel and hadi_fixing_kernel
// behind the listed steps.  Never shipped.
#include "emu_small_sch.cpp"

// Elements of the packed state of n_inst instances (0: no plan).
extern "C" long long emu_cliquet_packed_size(int n_inst, int m1, int m2) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 0;
    return (long long)pl.L.inst_stride * n_inst;
}

// Arrays natural layout [n][...].  par8 [n][8]: rho, sigma, kappa, eta, dt, N, strike, put -- the rows fill_desc builds; N and dt
// may differ between instances.  kind: 0 / 1 hadi_small_kernel with 4 / 8 wavefronts, 2 hadi_small_seq_kernel, 3
// hadi_small_seq2_kernel, 4 hadi_small_sch_kernel, 5 the streaming kernels (the plan's own choice; emu_set_tuning "strip" pins it).
// scheme: enum hadi_scheme.  U: the initial field (not modified); payoff: P (or NULL: U).  ref_spot, mode [n].  fix_steps
// [fix_rows][n_fix], fix_rows 1 or n, rows zero-padded; weights the same shape or NULL; n_fix = 0: no fixing tables at all (the plain
// call).  U_out [n][m].  P_out (or NULL) [emu_cliquet_packed_size]: the packed state the sweep leaves; is_pad (or NULL), same size:
// 1 where the element is no node (a pad slot, a slot of a node beyond m1, an identity row).  iref_out (or NULL) [2][n]: the located
// nodes and their status words.
// Returns 0, 1 (no plan), 2 (no such kernel), 3 (not admitted), 4 (device error word set).
extern "C" int emu_cliquet(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8, const double *vec_s,
                           const double *vec_v, const double *delta_s, const double *delta_v, const double *U, const double *payoff,
                           int kind, int scheme, int ndiv, const double *ddates, const double *damounts, const double *dpcts,
                           const double *ref_spot, const int *mode, int n_fix, const int *fix_steps, int fix_rows, const double *weights,
                           double *U_out, double *P_out, unsigned char *is_pad, int *iref_out) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    if (hadi_no_strips(theta, r_d == r_f)) pl.use_strip = 0;
    const HadiLayout &L = pl.L;
    const bool dividend = ndiv > 0, cs = scheme != 0;
    if (kind < 0 || kind > 5 || scheme < 0 || scheme > 3 || (fix_rows != 1 && fix_rows != n_inst)) return 3;
    if (kind == 4 && (!cs || !hadi_small_sch_admits(L) || dividend)) return 3;
    if (kind < 4 && (cs || !(pl.smem_small_eu > 0))) return 3;
    if (kind == 3 && L.nrows > 32) return 3;
    if (kind == 5 && cs && dividend) return 3;
    const size_t st = (size_t)L.inst_stride * n_inst;
    std::vector<double> dU(st), dY(st, 0.0), dUT(dividend ? st : 0), dV(cs ? st : 0), dR1(cs ? st : 0), dC2(cs ? st : 0);
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
    // the tables, as stage_dividends, stage_step_flags and stage_cliquet build them
    const int flag_stride = uniform ? 0 : Nmax, fix_stride = fix_rows > 1 ? Nmax : 0;
    std::vector<int> flags((size_t)(uniform ? 1 : n_inst) * Nmax, -1), fixf((size_t)(fix_stride ? n_inst : 1) * Nmax, 0);
    std::vector<double> wt(fixf.size(), 0.0);
    std::vector<char> div_step(Nmax + 1, 0), fix_step(Nmax + 1, 0);
    bool any_w = false;
    if (dividend)
        for (int k = 0; k < (uniform ? 1 : n_inst); k++) {
            int *f = flags.data() + (size_t)k * Nmax;
            hadi_dividend_steps((int)par8[(size_t)k * 8 + 5], par8[(size_t)k * 8 + 4], ndiv, ddates, f, Nmax);
            for (int q = 0; q < Nmax; q++)
                if (f[q] >= 0) div_step[q + 1] = 1;
        }
    for (int k = 0; k < (fix_stride ? n_inst : 1); k++)
        for (int q = 0; q < n_fix; q++) {
            const int n = fix_steps[(size_t)k * n_fix + q];
            if (n <= 0) continue;
            fixf[(size_t)k * Nmax + n - 1] = 1;
            fix_step[n] = 1;
            if (weights) wt[(size_t)k * Nmax + n - 1] = weights[(size_t)k * n_fix + q];
            any_w = any_w || (weights && weights[(size_t)k * n_fix + q] != 0.0);
        }
    // the packed payoff: only where some fixing carries a weight (HadiRoute::need_u0)
    std::vector<double> dP0(any_w ? st : 0, std::nan(""));
    if (any_w) emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, payoff ? payoff : U, dP0.data()); });
    std::vector<int> iref((size_t)2 * n_inst, -12345);
    if (n_fix > 0)
        emu::launch((n_inst + 63) / 64, 64, [&]() { hadi_fixing_locate_kernel(L, n_inst, vec_s, ref_spot, iref.data(), iref.data() + n_inst); });
    if (iref_out) std::copy(iref.begin(), iref.end(), iref_out);
    HadiSweepArgs a{};
    a.U = dU.data(); a.Y = dY.data();
    a.U0 = any_w ? dP0.data() : nullptr;
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw;
    a.bgroups = pl.bgroups; a.tile_il = g_tile_il; a.pos_m1 = pl.pos_m1; a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = &g_err; a.debug = g_debug;
    auto finish = [&]() {
        emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U_out); });
        if (P_out) std::copy(dU.begin(), dU.end(), P_out);
        if (is_pad)
            for (size_t e = 0; e < st; e++) {
                const size_t r = e % (size_t)L.inst_stride;
                const int i = hadi_slot_to_i(L, (int)(r % L.rowp));
                is_pad[e] = (i < 0 || i > L.m1 || (int)(r / L.rowp) >= L.nrows) ? 1 : 0;
            }
        return g_err ? 4 : 0;
    };
    if (kind < 5) {
        HadiSmallArgs sm;
        sm.div_flag = dividend ? flags.data() : nullptr; sm.flag_stride = flag_stride; sm.div_amounts = damounts; sm.div_pcts = dpcts;
        sm.vec_s = vec_s; sm.Nmax = Nmax;
        std::vector<int> order(n_inst);  // longest-processing-time-first dispatch order, as small_args builds it
        for (int k = 0; k < n_inst; k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return par8[(size_t)x * 8 + 5] > par8[(size_t)y * 8 + 5]; });
        sm.order = uniform ? nullptr : order.data();
        if (n_fix > 0) {
            sm.fix_flag = fixf.data(); sm.fix_stride = fix_stride; sm.fix_w = any_w ? wt.data() : nullptr;
            sm.fix_iref = iref.data(); sm.fix_mode = mode;
        }
        if (kind == 4) {
            const HadiLoopFn fn = hadi_small_sch_fn(L.B, hadi_route_sch(scheme));
            if (!fn) return 2;
            emu::launch(n_inst, 64, [&]() { fn(a, sm); }, hadi_small_sch_smem(L));
        } else {
            const HadiSel sel = hadi_select_small(pl, n_inst, kind == 3 ? 2 : kind == 2 ? 1 : 0, kind == 1 ? 8 : 4, false);
            if (!sel.k) return 2;
            emu::launch(sel.grid, sel.block, [&]() { sel.k->loop(a, sm); }, sel.smem);
        }
        return finish();
    }
    // the streaming loop of enqueue_sub_batch (one sub-batch, European sweeps with the fp64 state)
    std::vector<double> dW(pl.row_seq ? st : 0);
    a.R1 = cs ? dR1.data() : pl.row_seq ? dW.data() : nullptr; a.C2 = cs ? dC2.data() : nullptr;
    const bool pair_tab = hadi_pair_table(pl, cs) && pl.use_strip;
    std::vector<double> dRS(pair_tab ? (size_t)n_inst * L.nrows * 128 : 0, std::nan(""));
    a.rs_tab = pair_tab ? dRS.data() : nullptr;
    HadiSweepArgs av = a;
    if (cs) av.U = dV.data();
    if (pair_tab && run_pass(hadi_select_pair_table(pl), a, 1)) return 2;
    const int bpi = hadi_exercise_bpi(L), c_stride = L.nrows_pad;
    std::vector<double> cbuf((size_t)n_inst * c_stride, std::nan(""));
    for (int n = 1; n <= Nmax; n++) {
        if (dividend && div_step[n]) {
            dUT = dU;
            emu::launch(8, 64, [&]() {
                hadi_dividend_kernel(L, n_inst, ipar.data(), vec_s, dUT.data(), dU.data(), flags.data(), flag_stride, n, damounts, dpcts);
            });
        }
        const HadiPassCtx pc{pl, n_inst, false, false, false, false, scheme, g_cs_strips, g_col_prefetch};
        const HadiSel col = hadi_select_col_pass(pc);
        for (int md = cs ? 1 : 0; md <= (cs ? 2 : 0); md++)
            if (run_pass(hadi_select_row_pass(pc, md), md == 2 ? av : a, n) || run_pass(col, md == 1 ? av : a, n)) return 2;
        if (n_fix > 0 && fix_step[n]) {
            emu::launch((unsigned)((n_inst * L.nrows + 255) / 256), 256, [&]() {
                hadi_fixing_gather_kernel(L, n_inst, dU.data(), fixf.data(), fix_stride, iref.data(), cbuf.data(), c_stride, n);
            });
            emu::launch((unsigned)n_inst * bpi, HADI_EX_THREADS, [&]() {
                hadi_fixing_kernel(L, n_inst, bpi, dU.data(), any_w ? dP0.data() : nullptr, fixf.data(), any_w ? wt.data() : nullptr, fix_stride,
                                   iref.data(), mode, cbuf.data(), c_stride, vec_s, n);
            });
        }
    }
    return finish();
}

// emu_route (emu_driver.cpp) with the inputs a cliquet call adds: the number of its fixing steps and whether a weight is non-zero.
// o[17]: emu_route's 15 words, HadiRoute::cliquet and HadiRoute::need_u0.
extern "C" int emu_route_cliquet(const int *in, double theta, const char *tuning, int n_fix_steps, int fix_weights, long long *o, int *subs,
                                 int max_subs, char *desc, int cap) {
    HadiRouteIn ri;
    ri.cu_count = in[0]; ri.n = in[1]; ri.m1 = in[2]; ri.m2 = in[3]; ri.variant = in[4]; ri.scheme = in[5]; ri.prec = in[6];
    ri.theta = theta; ri.rates_equal = in[7] != 0; ri.debug = in[8]; ri.profiling = in[9] != 0; ri.n_snap = in[10];
    ri.dividends = in[11] != 0; ri.uniform_steps = in[12] != 0; ri.team_failed = in[13] != 0;
    ri.n_fix_steps = n_fix_steps; ri.fix_weights = fix_weights != 0;
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
    const long long v[17] = {r.status, r.kind, r.small_waves, (long long)r.bp.subs.size(), r.bp.two_streams, r.bp.fork_before, r.n_resident(),
                             r.read_payoff_shape, r.pair_tab, r.need_lam_u0, r.need_ut, r.need_f32, r.need_v_r1_c2, r.need_r1, r.graphable,
                             r.cliquet, r.need_u0};
    std::copy(v, v + 17, o);
    for (int k = 0; k < (int)r.bp.subs.size() && k < max_subs; k++) {
        const int s4[4] = {r.bp.subs[k].off, r.bp.subs[k].cnt, r.bp.subs[k].lane, r.resident[k]};
        std::copy(s4, s4 + 4, subs + 4 * k);
    }
    std::snprintf(desc, cap, "%s", hadi_describe_route(r, ri, in[14] != 0, in[15]).c_str());
    return 0;
}
