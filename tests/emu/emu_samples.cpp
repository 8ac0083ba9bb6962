// emu_samples.cpp -- TEST-ONLY.  The wave emulator's driver of the sampled ladder of the four whole-loop kernels: emu_ladder.cpp
// (included whole, so the plain ladder is in the same library) plus one entry point that builds the tables, packs the initial
// field, locates the samples as the library does (hadi_setup_kernel, hadi_pack_kernel, hadi_sample_locate_kernel), runs the
// kernel's whole time loop with the snapshot list and the tap table, and returns the samples.  emu_sample_field (below) runs the
// streaming path's sample kernels on given fields, without a sweep.  Never shipped.
#include "emu_ladder.cpp"

// The arguments of emu_ladder with the samples in S_0's place: spots / scales [rows][n_samp] (scales may be NULL = 1), rows 1 or
// n_inst, expanded to one row per instance as the library's staging does.  out [n][n_snap][n_samp]: the samples; flags
// [n][n_samp]: the locate kernel's words.  Returns what emu_ladder returns.
extern "C" int emu_samples(int n_inst, int m1, int m2, double theta, double r_d, double r_f, const double *par8,
                           const double *vec_s, const double *vec_v, const double *delta_s, const double *delta_v,
                           const double *U, const double *U0, int kind, int variant, int scheme, int ndiv, const double *ddates,
                           const double *damounts, const double *dpcts, double V_0, int n_samp, const double *spots,
                           const double *scales, int rows, int n_snap, const int *snap_steps, double *out, int *flags) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    const HadiLayout &L = pl.L;
    const int american = variant & 1, dividend = (variant >> 1) & 1;
    if (kind < 0 || kind > 4) return 3;
    if (american && kind > 1) return 3;
    if (kind == 4 && (scheme < 1 || scheme > 3 || !hadi_small_sch_admits(L) || american || dividend)) return 3;
    if (kind < 4 && (scheme != 0 || !((american ? pl.smem_small_am : pl.smem_small_eu) > 0))) return 3;
    if (kind == 3 && L.nrows > 32) return 3;
    if (n_samp < 1 || (rows != 1 && rows != n_inst)) return 3;
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
    // the lists of all instances, then the tap records
    const size_t ns = (size_t)n_inst * n_samp;
    std::vector<double> in(2 * ns);
    for (int k = 0; k < n_inst; k++)
        for (int q = 0; q < n_samp; q++) {
            const size_t src = (size_t)(rows > 1 ? k : 0) * n_samp + q;
            in[(size_t)k * n_samp + q] = spots[src];
            in[ns + (size_t)k * n_samp + q] = scales ? scales[src] : 1.0;
        }
    std::vector<HadiTap> taps(ns);
    std::vector<int> node(n_inst, -1);
    emu::launch((int)((ns + 255) / 256), 256, [&]() {
        hadi_sample_locate_kernel(L, n_inst, n_samp, vec_s, vec_v, (const double *)nullptr, V_0, in.data(), in.data() + ns, taps.data(), flags);
    });
    HadiSweepArgs a{};
    a.U = dU.data(); a.LAM = american ? dLAM.data() : nullptr; a.U0 = american ? dU0.data() : nullptr;
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.pos_m1 = pl.pos_m1; a.american = american;
    a.err = &g_err; a.debug = g_debug;
    const int N = (int)par8[5];
    for (int k = 0; k < n_inst; k++)
        if ((int)par8[(size_t)k * 8 + 5] != N) return 3;
    std::vector<int> dflags((size_t)n_inst * N, -1);
    if (dividend)
        for (int k = 0; k < n_inst; k++) hadi_dividend_steps(N, par8[(size_t)k * 8 + 4], ndiv, ddates, dflags.data() + (size_t)k * N, N);
    std::vector<double> snap_out((size_t)n_inst * n_snap, 0.0);  // (the single node's output: must stay untouched)
    HadiSmallArgs sm;
    sm.div_flag = dividend ? dflags.data() : nullptr; sm.flag_stride = N; sm.div_amounts = damounts; sm.div_pcts = dpcts;
    sm.vec_s = vec_s; sm.Nmax = N; sm.order = nullptr;
    sm.snap_steps = snap_steps; sm.n_snap = n_snap; sm.snap_node = node.data(); sm.snap_out = snap_out.data();
    sm.taps = taps.data(); sm.n_samp = n_samp; sm.samp_out = out;
    if (kind == 4) {
        const HadiLoopFn fn = hadi_small_sch_fn(L.B, scheme == 2 ? HADI_SCH_MCS : scheme == 3 ? HADI_SCH_HV : HADI_SCH_CS);
        if (!fn) return 2;
        emu::launch(n_inst, 64, [&]() { fn(a, sm); }, hadi_small_sch_smem(L));
    } else {
        const HadiSel sel = hadi_select_small(pl, n_inst, kind == 3 ? 2 : kind == 2 ? 1 : 0, kind == 1 ? 8 : 4, american != 0);
        if (!sel.k) return 2;
        emu::launch(sel.grid, sel.block, [&]() { sel.k->loop(a, sm); }, sel.smem);
    }
    for (double x : snap_out)
        if (x != 0.0) return 5;
    return g_err ? 4 : 0;
}

// The streaming path's three sample kernels on ANY layout, without a sweep: the plan, hadi_pack_kernel on given fields,
// hadi_sample_locate_kernel over the whole batch, then hadi_sample_kernel once per sub-batch and snapshot with the offsets
// run_sweep (hadi_api.hip) gives a sub-batch of nsb instances starting at instance o: the state at o * inst_stride, the tap
// records at o * n_samp, the samples at o * n_snap * n_samp.  fields [n_snap][n][m] in natural order: the state "after" snapshot
// step q.  V0_i [n] or NULL (then V_0).  sub [n_sub]: the sub-batch sizes, summing to n_inst.  spots / scales [rows][n_samp], rows
// 1 or n_inst (scales may be NULL).  out [n][n_snap][n_samp], flags [n][n_samp].  Returns 0, 1 (no plan), 3 (bad arguments).
extern "C" int emu_sample_field(int m1, int m2, int n_inst, const double *vec_s, const double *vec_v, double V_0, const double *V0_i,
                                const double *fields, const double *spots, const double *scales, int rows, int n_samp, int n_snap,
                                const int *sub, int n_sub, double *out, int *flags) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    const HadiLayout &L = pl.L;
    if (n_samp < 1 || n_snap < 1 || (rows != 1 && rows != n_inst) || n_sub < 1) return 3;
    int sum = 0;
    for (int b = 0; b < n_sub; b++) {
        if (sub[b] < 1) return 3;
        sum += sub[b];
    }
    if (sum != n_inst) return 3;
    const size_t ns = (size_t)n_inst * n_samp, m = (size_t)(m1 + 1) * (m2 + 1);
    std::vector<double> in(2 * ns);
    for (int k = 0; k < n_inst; k++)
        for (int q = 0; q < n_samp; q++) {
            const size_t src = (size_t)(rows > 1 ? k : 0) * n_samp + q;
            in[(size_t)k * n_samp + q] = spots[src];
            in[ns + (size_t)k * n_samp + q] = scales ? scales[src] : 1.0;
        }
    std::vector<HadiTap> taps(ns);
    emu::launch((int)((ns + 255) / 256), 256, [&]() {
        hadi_sample_locate_kernel(L, n_inst, n_samp, vec_s, vec_v, V0_i, V_0, in.data(), in.data() + ns, taps.data(), flags);
    });
    std::vector<double> dU((size_t)L.inst_stride * n_inst);
    for (int q = 0; q < n_snap; q++) {
        emu::launch(8, 256, [&]() { hadi_pack_kernel(L, n_inst, n_inst, fields + (size_t)q * n_inst * m, dU.data()); });
        int o = 0;
        for (int b = 0; b < n_sub; o += sub[b], b++) {
            const int nsb = sub[b];
            const size_t nsq = (size_t)nsb * n_samp;
            const double *Ub = dU.data() + (size_t)o * L.inst_stride;
            emu::launch((int)((nsq + 255) / 256), 256, [&]() {
                hadi_sample_kernel(L, nsb, Ub, taps.data() + (size_t)o * n_samp, out + (size_t)o * n_snap * n_samp, n_snap, n_samp, q);
            });
        }
    }
    return 0;
}

// Layout words of the plan of a shape, for the tests' own assertions: B, G, rowp, nrows_pad.
extern "C" int emu_sample_layout(int m1, int m2, int n_inst, int *o4) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * 256, &pl, g_tune, 8)) return 1;
    o4[0] = pl.L.B; o4[1] = pl.L.G; o4[2] = pl.L.rowp; o4[3] = pl.L.nrows_pad;
    return 0;
}
