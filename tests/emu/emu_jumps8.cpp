// emu_jumps8.cpp -- TEST-ONLY.  The wave emulator's driver of the nine-group batch of hadi_compute_jacobian_bates_jumps:
// emu_jumps.cpp (included whole) plus one entry point that builds the weights and the three matrix sets as apply_extras /
// stage_jumps of hadi_api.hip do and runs the streaming loop of enqueue_sub_batch with the copy of U and hadi_jump_sel_kernel
// behind every step's last column pass.  Never shipped.
#include "emu_jumps.cpp"

// The batch is 9 groups of n0 source instances.  Arrays natural layout; par8, vec_s, vec_v, delta_s, delta_v hold all 9 n0 rows as
// jacobian_common / jacobian_grids leave them (the caller's rows repeated, the bumped parameters, group 5's v-grid rebuilt); U
// [n0][m]: the initial field of the source instances (not modified).  lam, mu, sig [n0]; eps: the Jacobian's step.  shared: one
// matrix per set, built on the rows 0, 1, 2 with (mu[0], sig[0]).  share, cap: HadiJumpSel's (the library: jump_sel).  split: the
// batch runs as the two launches [0, split) and [split, 9 n0) per step, as two sub-batches do (0: one launch).
// U_out [9 n0][m]; P_out / is_pad (or NULL) as emu_jumps has them.
// Returns 0, 1 (no plan), 2 (no such kernel), 3 (not admitted), 4 (device error word set).
extern "C" int emu_jumps8(int n0, int m1, int m2, double theta, double r_d, double r_f, const double *par8, const double *vec_s,
                          const double *vec_v, const double *delta_s, const double *delta_v, const double *U, int scheme,
                          const double *lam, const double *mu, const double *sig, double eps, int shared, int share, int cap, int split,
                          double *U_out, double *P_out, unsigned char *is_pad) {
    const int n_inst = HADI_JUMP_GROUPS * n0;
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    if (hadi_no_strips(theta, r_d == r_f)) pl.use_strip = 0;
    const HadiLayout &L = pl.L;
    const bool cs = scheme != 0;
    if (scheme < 0 || scheme > 3 || pl.row_seq || pl.col_seq || cap < 1 || cap > 8 || split < 0 || split >= n_inst || (share && shared)) return 3;
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
    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n0, U, dU.data()); });
    int Nmax = 0;
    for (int k = 0; k < n_inst; k++) Nmax = std::max(Nmax, (int)par8[(size_t)k * 8 + 5]);
    // the weights and the three matrix sets, as apply_extras and stage_jumps build them
    std::vector<double> avec(n_inst), musig;
    for (int k = 0; k < n_inst; k++) avec[k] = (k / n0 == 6 ? lam[k % n0] + eps : lam[k % n0]) * par8[(size_t)k * 8 + 4];
    const int per = shared ? 1 : n0, n_mat = HADI_JUMP_SETS * per;
    for (int q = 0; q < n_mat; q++) {
        musig.push_back(mu[q % per] + (q / per == 1 ? eps : 0.0));
        musig.push_back(sig[q % per] + (q / per == 2 ? eps : 0.0));
    }
    std::vector<double> G((size_t)n_mat * hadi_jump_matrix_doubles(L), 0.0);
    const size_t ne = (size_t)n_mat * (m1 + 1) * (m1 + 1);
    emu::launch((unsigned)((ne + 255) / 256), 256, [&]() { hadi_jump_matrix_kernel(L, n_mat, vec_s, musig.data(), G.data()); });
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
        const HadiPassCtx pc{pl, n_inst, false, false, false, false, scheme, g_cs_strips, g_col_prefetch};
        const HadiSel col = hadi_select_col_pass(pc);
        for (int mode = cs ? 1 : 0; mode <= (cs ? 2 : 0); mode++)
            if (run_pass(hadi_select_row_pass(pc, mode), mode == 2 ? av : a, n) || run_pass(col, mode == 1 ? av : a, n)) return 2;
        dUT = dU;  // U_temp <- U, then the sub-step out of place, sub-batch by sub-batch
        const int cuts[3] = {0, split ? split : n_inst, n_inst};
        for (int sb = 0; sb < (split ? 2 : 1); sb++) {
            const int o = cuts[sb], nsb = cuts[sb + 1] - o;
            const size_t so = (size_t)o * L.inst_stride;
            const HadiJumpSel js{o, n0, per, share, cap};
            emu::launch(hadi_jump_sel_grid(L, js, nsb), HADI_JUMP_THREADS, [&]() {
                hadi_jump_sel_kernel(L, nsb, js, dUT.data() + so, dU.data() + so, G.data(), (long long)hadi_jump_matrix_doubles(L),
                                     avec.data() + o, ipar.data() + o, n);
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

// The lists of hadi_jump_sel_kernel for one launch: how often each instance of the launch appears (cover [n_inst], zeroed here)
// and the largest list.  Returns the number of lists, or -1 when a list names an instance outside the launch.
extern "C" int emu_jump_sel_lists(int inst0, int n_src, int per, int share, int cap, int n_inst, int *cover, int *longest) {
    const HadiJumpSel q{inst0, n_src, per, share, cap};
    const int ngrp = hadi_jump_sel_ngrp(q, n_inst);
    std::fill(cover, cover + n_inst, 0);
    *longest = 0;
    for (int grp = 0; grp < ngrp; grp++) {
        const HadiJumpList li = hadi_jump_sel_list(q, n_inst, grp);
        *longest = std::max(*longest, li.count);
        int mat = -1;
        for (int c = 0; c < li.count; c++) {
            const int inst = li.start + c * li.stride;
            if (inst < 0 || inst >= n_inst) return -1;
            cover[inst]++;
            const int k = inst0 + inst, g = k / n_src, m = hadi_jump_set(g) * per + (per > 1 ? k % n_src : 0);
            if (share && c > 0 && m != mat) return -1;  // (a shared strip: one matrix per list)
            mat = m;
        }
    }
    return ngrp;
}
