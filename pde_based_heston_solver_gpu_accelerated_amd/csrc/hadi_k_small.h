// hadi_k_small.h -- LDS-resident kernels of the calibration-size grids: hadi_small_kernel (a block of 4 or 8 wavefronts per
// instance, the big-grid row step on LDS rows) and hadi_small_seq_kernel / hadi_small_seq2_kernel (one wavefront per instance /
// per pair of instances, lines solved sequentially).  The two sequential kernels include one row sweep (hadi_k_lds_row_body.h) and
// take the rest from hadi_k_lds_seq.h (stage-in / stage-out, the lane's row-table entry, the back substitution, the column
// sweep); the dividend jump's value of all three is hadi_dividend_jump (hadi_k_common.h).
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// ------------------------------------------------------------------------------------------------
// Small grids (the reference's calibration / perf-harness sizes, e.g. 50x25: perfomance_test.cpp:46-57):
// the whole instance lives in LDS and ONE launch runs the entire time loop -- no HBM traffic and no kernel
// boundaries inside the loop.  Block = W wavefronts <-> one instance (W = 4: measured faster than 16 on MI355X,
// 0.37 vs 0.46 ms for 500 instances of 50x25x20 -- more blocks per CU beat more waves per instance).  Per step: the row pass is the same
// hadi_row_step as above (rows taken straight from the LDS-resident state, Y written to LDS), then the
// column pass walks each column sequentially in LDS (single chunk: m2+1 <= HADI_LC), with the American
// projection; discrete dividends are applied in place.
struct HadiSmallArgs {
    const int *div_flag;        // dividend index applied at the START of step n (n = 1..Nmax), or -1; nullptr = none.
                                // Instance k reads div_flag[k*flag_stride + n-1]: flag_stride 0 = one shared (N, dt)
    int flag_stride;
    const double *div_amounts;  // device copies of the schedule
    const double *div_pcts;
    const double *vec_s;        // [n_inst][m1+1] (dividend interpolation)
    int Nmax;
    const int *order;           // block b solves instance order[b] (longest time loops first), nullptr = identity
    // Maturity ladder (hadi_maturity_ladder; 0 / nullptr = none): after step snap_steps[q] (strictly increasing, device array)
    // the value of node snap_node[inst] -- the packed offset row * rowp + slot that hadi_locate_kernel wrote, -1 if S_0 is off the
    // instance's s-grid -- goes to snap_out[inst * n_snap + q]
    const int *snap_steps = nullptr;
    int n_snap = 0;
    const int *snap_node = nullptr;
    double *snap_out = nullptr;
    // Bermudan exercise (hadi_bermudan_timestepping; nullptr = none): instance k takes U <- max(U, payoff) at the END of step n
    // where ex_flag[k*ex_stride + n-1] != 0 (ex_stride 0 = one shared row).  The payoff is HadiSweepArgs::U0 (packed, global).
    const int *ex_flag = nullptr;
    int ex_stride = 0;
    // Knock-out barrier (hadi_barrier_timestepping; nullptr = none): at the END of step n where ko_flag[k*ko_stride + n-1] != 0
    // (ko_stride 0 = one shared row) instance k takes U <- ko_rebate[k] on the nodes outside ko_iab[2k] .. ko_iab[2k+1], the live
    // index range that hadi_barrier_locate_kernel wrote
    const int *ko_flag = nullptr;
    int ko_stride = 0;
    const int *ko_iab = nullptr;
    const double *ko_rebate = nullptr;
    // Strike fixings (hadi_cliquet_timestepping; nullptr = none): at the END of step n where fix_flag[k*fix_stride + n-1] != 0
    // (fix_stride 0 = one shared row) instance k takes U(i, j) <- a_i U(fix_iref[k], j) + w P(i, j) with w = fix_w[k*fix_stride + n-1]
    // (nullptr: 0), a_i by fix_mode[k] (hadi_k_fixing.h); fix_iref is what hadi_fixing_locate_kernel wrote, P is HadiSweepArgs::U0
    const int *fix_flag = nullptr;
    int fix_stride = 0;
    const double *fix_w = nullptr;
    const int *fix_iref = nullptr;
    const int *fix_mode = nullptr;
    // Sampled ladder (hadi_sample_ladder; n_samp 0 = none): on the snapshot steps above, instead of the one node, sample s of the
    // instance -- the tap record taps[inst * n_samp + s] that hadi_sample_locate_kernel wrote -- goes to
    // samp_out[(inst * n_snap + q) * n_samp + s]
    const HadiTap *taps = nullptr;
    int n_samp = 0;
    double *samp_out = nullptr;
    // Lognormal jumps (hadi_bates_sample_ladder; nullptr = none, hadi_small_jump_kernel only): at the END of every step n <= N_k,
    // behind the column pass and in front of the snapshot, instance k with jmp_a[k] != 0 takes U_row <- U_row + jmp_a[k] (G U_row)
    // on every v-row, G the matrix jmp_mat[k] of jmp_G (operand order, hadi_k_jumps.h; jmp_stride doubles per matrix)
    const double *jmp_G = nullptr;
    const double *jmp_a = nullptr;
    const int *jmp_mat = nullptr;
    long long jmp_stride = 0;
};

// The ladder's running cursor of a whole-loop kernel: wave-uniform (kernel arguments and the step counter only).  `next` is the
// step of the next snapshot, 0 when none is left (no step is numbered 0).
struct HadiSnapCursor {
    int q, next;
};
HADI_HD inline HadiSnapCursor hadi_snap_begin(const HadiSmallArgs &sm) {
    return HadiSnapCursor{0, sm.n_snap > 0 ? sm.snap_steps[0] : 0};
}
HADI_HD inline void hadi_snap_advance(const HadiSmallArgs &sm, HadiSnapCursor &sc) {
    sc.q++;
    sc.next = sc.q < sm.n_snap ? sm.snap_steps[sc.q] : 0;
}
// The node's offset in an LDS field kept in natural order with pitch PL (the sequential kernels), from the packed offset
HADI_HD inline int hadi_snap_natural(const HadiLayout &L, int node, int PL) {
    if (node < 0) return -1;
    const int j = node / L.rowp, i = hadi_slot_to_i(L, node - j * L.rowp);
    return i < 0 ? -1 : j * PL + i;
}
// Sampled ladder: snapshot q of instance `inst` from its LDS field Ul -- packed as the global state is, or (natural) in natural
// order with pitch PL.  Lanes first, first + stride, .. take the samples; the tap records are read from the global table here, on
// snapshot steps only, as the Bermudan payoff is.  `on`: this lane serves the instance (the halves of the pairs kernel).
HADI_DEV inline void hadi_sample_lds(const HadiSmallArgs &sm, const HadiLayout &L, const double *Ul, bool natural, int PL, int inst,
                                     int q, int first, int stride, bool on) {
    if (!on) return;
    const HadiTap *__restrict__ tp = sm.taps + (size_t)inst * sm.n_samp;
    double *__restrict__ out = sm.samp_out + ((size_t)inst * sm.n_snap + q) * sm.n_samp;
    for (int s = first; s < sm.n_samp; s += stride) {
        const HadiTap t = tp[s];
        out[s] = hadi_tap_value(t, [&](int off) { return Ul[natural ? hadi_snap_natural(L, off, PL) : off]; });
    }
}

// The jump sub-step of a whole-loop kernel, hadi_jump_step's product on the LDS-resident state: Ul <- Yl + a G Yl on every v-row,
// Yl the copy of U that the caller made (out of place: every tile reads whole rows of the old field).  One 16-row x 16-output-slot
// accumulator tile per wavefront at a time, the (row block, slot block) tiles dealt round-robin over the W wavefronts; the K loop
// runs over ALL kg groups of 4 input slots in ascending slot order, the padding included -- the very sequence of matrix
// instructions hadi_jump_step issues for the tile, so an instance's sub-step does not depend on the route.  A: lane 16 k + j reads
// Yl[(j0 + j) rowp + k0 + k], masked as hadi_jump_step's fetch masks (rows >= nrows, slots past the pitch and slots that hold no
// node read as 0.0: behind Yl's nrows rows lie other tables, and the pad slots hold what the column pass left there).  B: the 64
// contiguous doubles of G's (block, group) cell straight from global memory (one coalesced 512-byte cell per instruction; a
// matrix is 61 KB at 50x25 and stays in L2), a chunk of HADI_JUMP_KC / 4 cells in flight ahead of the matrix core.
// Never written: pad slots, slots beyond m1, the halo rows.  Row i = 0 of G is zero: that column keeps its bits.
template <int W>
HADI_DEV HADI_FORCEINLINE void hadi_small_jump_stage(const HadiLayout &L, const double *Yl, double *Ul, const double *__restrict__ Gm,
                                                     double a, int wave, int lane) {
    // cells per chunk (kg is a multiple of it).  Measured (profiles/bates_surface_ab.txt): a tile's whole strip in flight at once --
    // 24 or 40 cells -- was SLOWER than this chunk of 8 with the next chunk's loads behind it (one 50x25 instance x 100 steps 1.94 ->
    // 2.10 ms, 100x20 3.63 -> 4.13 ms), and was not kept.
    constexpr int KC = HADI_JUMP_KC / 4;
    const int kg = hadi_jump_kg(L), nib = hadi_jump_nib(L), rowp = L.rowp, nrows = L.nrows;
    const int ntiles = ((nrows + 15) / 16) * nib;
    for (int t = wave; t < ntiles; t += W) {  // (wave-uniform)
        const int rb = t / nib, sb = t - rb * nib;
        const double *__restrict__ bp = Gm + (size_t)sb * kg * 64 + lane;
        const int ja = 16 * rb + (lane & 15);  // the row of this lane's A operands
        const double *ap = Yl + (size_t)(ja < nrows ? ja : 0) * rowp;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        double bn[KC], bc[KC];
#pragma unroll
        for (int kk = 0; kk < KC; kk++) bn[kk] = bp[64 * kk];
        for (int g0 = 0; g0 < kg; g0 += KC) {
#pragma unroll
            for (int kk = 0; kk < KC; kk++) bc[kk] = bn[kk];
            if (g0 + KC < kg) {
#pragma unroll
                for (int kk = 0; kk < KC; kk++) bn[kk] = bp[(size_t)64 * (g0 + KC + kk)];
            }
#pragma unroll
            for (int kk = 0; kk < KC; kk++) {
                const int sl = 4 * (g0 + kk) + (lane >> 4);
                const int il = sl < rowp ? hadi_slot_to_i(L, sl) : -1;
                const bool ok = ja < nrows && il >= 0 && il <= L.m1;
                double av = 0.0;
                if (ok) av = ap[sl];
                hadi_mfma_f64_16x16x4(av, bc[kk], acc);
            }
        }
        const int so = 16 * sb + (lane & 15), io = so < rowp ? hadi_slot_to_i(L, so) : -1;
        const bool so_ok = io >= 0 && io <= L.m1;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = 16 * rb + 4 * r + (lane >> 4);
            if (so_ok && j < nrows) {
                const size_t off = (size_t)j * rowp + so;
                Ul[off] = Yl[off] + a * acc[r];
            }
        }
    }
}

// The time loop of hadi_small_kernel and, with JUMP, of hadi_small_jump_kernel (one more stage between the column pass and the
// snapshot; European sweeps only).
template <int B, int W, bool AMER, bool JUMP>
HADI_DEV HADI_FORCEINLINE void hadi_small_body(const HadiSweepArgs &a, const HadiSmallArgs &sm) {
    static_assert(!(AMER && JUMP), "the jump stage belongs to European sweeps");
    HADI_DYN_SMEM(double, smem);
    constexpr int G = 1, NT = 64 * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = HADI_UNIFORM((int)(threadIdx.x >> 6));
    if ((int)blockIdx.x >= a.n_inst) return;
    // multi-maturity batches: instances with many time steps are dispatched first, short ones fill the tail
    const int inst = sm.order ? sm.order[blockIdx.x] : (int)blockIdx.x;
    const HadiInstPar ip = a.ipar[inst];
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1;
    constexpr int c0slot = 64 * B;
    // LDS map: U with two zero rows above and below, Y, [lambda, payoff], coefficients, row table, column table
    const int rows_l = nrows + 4;
    double *Ul = smem + 2 * rowp;                 // row 0 of U (rows -2, -1 and nrows, nrows+1 are zero)
    double *Yl = smem + (size_t)rows_l * rowp;    // nrows rows
    double *LAMl = Yl + (size_t)nrows * rowp;
    double *U0l = LAMl + (AMER ? (size_t)nrows * rowp : 0);
    double *coef = U0l + (AMER ? (size_t)nrows * rowp : 0);
    double *rtab = coef + 4 * 64 * B;
    double *ptab = rtab + (size_t)nrows * HADI_RCL;

    double *__restrict__ Ug = a.U + (size_t)inst * a.L.inst_stride;
    // zero the halo rows of U and ALL of Y: the column pass also sweeps the pad slots of every row, which the row pass
    // never writes -- whatever LDS held there (possibly NaN) would reach U's pad slot, and lane 63 multiplies that slot
    // by a zero coefficient (NaN * 0 = NaN)
    for (int e = tid; e < (rows_l + nrows) * rowp; e += NT) smem[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < nrows * rowp; e += NT) Ul[e] = Ug[e];
    if constexpr (AMER) {
        const double *__restrict__ P0g = a.U0 + (size_t)inst * a.L.inst_stride;
        for (int e = tid; e < nrows * rowp; e += NT) {
            U0l[e] = P0g[e];
            LAMl[e] = 0.0;  // lambda_bar <- 0, device_solver.hpp:310-313
        }
    }
    {
        const double *__restrict__ sc = a.scoef + (size_t)inst * 4 * 64 * B;
        for (int e = tid; e < 4 * 64 * B; e += NT) coef[e] = sc[e];
        const double *__restrict__ rg = a.rowc + (size_t)inst * nrows * HADI_RC;
        for (int e = tid; e < nrows * HADI_RCL; e += NT) rtab[e] = rg[(e / HADI_RCL) * HADI_RC + e % HADI_RCL];
        const double *__restrict__ pg = a.pb + (size_t)inst * a.L.nrows_pad * HADI_PBW;
        for (int e = tid; e < nrows * HADI_PBW; e += NT) ptab[e] = pg[e];
    }
    HadiRowCtx c;
    c.lane = lane; c.half = 0; c.wrow = wave; c.rowp = rowp;
    c.dt = ip.dt; c.thdt = ip.thdt; c.qd = ip.q; c.half_rd = ip.half_rd;
    c.hr0 = ip.hr0; c.inv0 = 1.0 / (1.0 + ip.thdt * ip.hr0);
    c.Yi = Yl; c.Li = AMER ? LAMl : nullptr;
    c.rowc = rtab; c.j0 = 0;
    c.b2r = a.b2row + (size_t)inst * rowp;
    c.coef = coef; c.xch = nullptr; c.R1i = nullptr; c.C2i = nullptr; c.err = a.err; c.debug = 0;
    c.payrow = nullptr; c.inv_dt = 0.0; c.m1_lane = -1; c.m1_r = -1;
    {
        const int ifirst = 1 + B * lane;
        c.posL = hadi_pos(B, G, ifirst - 1);
        c.posR = (ifirst + B <= 64 * B) ? hadi_pos(B, G, ifirst + B) : c0slot + 1;
    }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    unsigned long long stamp_store_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    c.stamp_acc_ = stamp_store_;
#endif
    __syncthreads();

    const int N = ip.N < sm.Nmax ? ip.N : sm.Nmax;
    HadiSnapCursor snap = hadi_snap_begin(sm);
    const int snap_off = sm.n_snap > 0 ? sm.snap_node[inst] : -1;
    HADI_STAMP_DECL(c.stamp_acc_)
    const double *__restrict__ vs = sm.vec_s ? sm.vec_s + (size_t)inst * (m1 + 1) : nullptr;
    [[maybe_unused]] const double jmp_a = (JUMP && sm.jmp_a) ? sm.jmp_a[inst] : 0.0;
    [[maybe_unused]] const double *__restrict__ jmp_Gm = (JUMP && sm.jmp_a) ? sm.jmp_G + (size_t)sm.jmp_mat[inst] * sm.jmp_stride : nullptr;
    for (int n = 1; n <= N; n++) {
        // ---- discrete dividend at the start of the step (device_solver.hpp:448-504) ---------------
        const int dv = sm.div_flag ? sm.div_flag[(size_t)inst * sm.flag_stride + n - 1] : -1;
        if (dv >= 0) {
            for (int e = tid; e < nrows * rowp; e += NT) Yl[e] = Ul[e];  // U_temp
            __syncthreads();
            const double amount = sm.div_amounts[dv], pct = sm.div_pcts[dv];
            for (int e = tid; e < nrows * (m1 + 1); e += NT) {
                const int j = e / (m1 + 1), i = e - j * (m1 + 1);
                const double *src = Yl + (size_t)j * rowp;
                Ul[(size_t)j * rowp + hadi_pos(B, G, i)] =
                    hadi_dividend_jump(vs, m1, amount, pct, ip.put, i, [&](int k) { return src[hadi_pos(B, G, k)]; });
            }
            __syncthreads();
        }
        // ---- row pass: 4 rows at a time, straight out of LDS -----------------------------------------
        c.e_nm1 = exp(ip.bc_rate * ip.dt * (n - 1));
        c.e_n = exp(ip.bc_rate * ip.dt * n);
        HADI_STAMP(8);
        for (int J = 0; J < nrows; J += W) {
            const int j = J + wave;
            if (j < nrows) {
                const double *r0 = Ul + (size_t)j * rowp;
                if (j == nrows - 1)
                    hadi_row_step<B, G, AMER, true>(c, true, j, r0 - 2 * rowp, r0 - rowp, r0, r0 + rowp, r0 + 2 * rowp);
                else
                    hadi_row_step<B, G, AMER, false>(c, true, j, r0 - 2 * rowp, r0 - rowp, r0, r0 + rowp, r0 + 2 * rowp);
            }
        }
        HADI_STAMP(10);  // row pass
        __syncthreads();
        HADI_STAMP(9);  // barrier
        // ---- column pass: one thread per storage column, sequential pentadiagonal sweeps in LDS --------
        for (int col = tid; col < rowp; col += NT) {
            // rounds of eight rows: the independent LDS reads first, then the dependent recurrence (as in hadi_small_seq_kernel)
            double ym1 = 0.0, ym2 = 0.0;
            int k = 0;
            for (; k + 8 <= nrows; k += 8) {
                double yv[8];
#pragma unroll
                for (int q = 0; q < 8; q++) yv[q] = Yl[(size_t)(k + q) * rowp + col];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const double *t = ptab + (size_t)(k + q) * HADI_PBW;
                    const double yk = (yv[q] - t[PB_L] * ym1 - t[PB_L2] * ym2) * t[PB_Q];
                    Yl[(size_t)(k + q) * rowp + col] = yk;
                    ym2 = ym1;
                    ym1 = yk;
                }
            }
            for (; k < nrows; k++) {
                const double *t = ptab + (size_t)k * HADI_PBW;
                const double yk = (Yl[(size_t)k * rowp + col] - t[PB_L] * ym1 - t[PB_L2] * ym2) * t[PB_Q];
                Yl[(size_t)k * rowp + col] = yk;
                ym2 = ym1;
                ym1 = yk;
            }
            double xp1 = 0.0, xp2 = 0.0;
            k = nrows - 1;
            if constexpr (!AMER) {
                for (; k >= 7; k -= 8) {
                    double yv[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) yv[q] = Yl[(size_t)(k - q) * rowp + col];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const double *t = ptab + (size_t)(k - q) * HADI_PBW;
                        const double xk = yv[q] - t[PB_C] * xp1 - t[PB_C2] * xp2;
                        xp2 = xp1;
                        xp1 = xk;
                        Ul[(size_t)(k - q) * rowp + col] = xk;
                    }
                }
            }
            for (; k >= 0; k--) {
                const double *t = ptab + (size_t)k * HADI_PBW;
                const double xk = Yl[(size_t)k * rowp + col] - t[PB_C] * xp1 - t[PB_C2] * xp2;
                xp2 = xp1;
                xp1 = xk;
                if constexpr (AMER) {  // Ikonen-Toivanen projection, device_solver.hpp:358-372
                    const size_t off = (size_t)k * rowp + col;
                    const double lamv = LAMl[off], pay = U0l[off];
                    Ul[off] = fmax(xk - ip.dt * lamv, pay);
                    double ln = fmax(0.0, lamv + (pay - xk) / ip.dt);
                    if (col == a.pos_m1) ln = 0.0;
                    LAMl[off] = ln;
                } else {
                    Ul[(size_t)k * rowp + col] = xk;
                }
            }
        }
        __syncthreads();
        if constexpr (JUMP) {  // Bates: the jump sub-step behind the column pass (block-uniform; n <= N_k inside this loop)
            if (jmp_a != 0.0) {
                // Y is dead behind the column pass: it takes the copy of U.  Only slots that hold a node are copied (the others are
                // never read here), so Y's pad slots stay what a sweep without jumps has there.
                for (int e = tid; e < nrows * rowp; e += NT) {
                    const int i = hadi_slot_to_i(a.L, e % rowp);
                    if (i >= 0 && i <= m1) Yl[e] = Ul[e];
                }
                __syncthreads();
                hadi_small_jump_stage<W>(a.L, Yl, Ul, jmp_Gm, jmp_a, wave, lane);
                __syncthreads();
            }
        }
        if constexpr (!AMER) {  // Bermudan exercise at the end of the step (European sweeps only; block-uniform)
            if (hadi_ex_listed(sm.ex_flag, sm.ex_stride, inst, n)) {
                hadi_exercise_lds<B>(Ul, rowp, false, a.U0 + (size_t)inst * a.L.inst_stride, nrows, m1, rowp, tid, NT);
                __syncthreads();
            }
            if (hadi_ex_listed(sm.ko_flag, sm.ko_stride, inst, n)) {  // knock-out at the end of a monitoring step (block-uniform)
                hadi_knock_lds<B>(Ul, rowp, false, sm.ko_iab[2 * inst], sm.ko_iab[2 * inst + 1], sm.ko_rebate[inst], nrows, m1, tid, NT);
                __syncthreads();
            }
            if (hadi_ex_listed(sm.fix_flag, sm.fix_stride, inst, n)) {  // strike fixing at the end of a fixing step (block-uniform)
                hadi_fixing_lds<B>(Ul, rowp, false, a.U0 + (size_t)inst * a.L.inst_stride, sm.vec_s + (size_t)inst * (m1 + 1), sm.fix_iref[inst],
                                   sm.fix_mode[inst], hadi_fix_weight(sm.fix_w, sm.fix_stride, inst, n), nrows, m1, rowp, tid, NT);
                __syncthreads();
            }
        }
        // maturity ladder: nothing writes U before the next barrier (the row pass reads it, a dividend copies it to Y first)
        if (n == snap.next) {
            if (sm.n_samp > 0) {  // sampled ladder: W wavefronts read arbitrary nodes of U, which nothing writes before the next barrier either
                hadi_sample_lds(sm, a.L, Ul, false, rowp, inst, snap.q, tid, NT, true);
                __syncthreads();
            } else if (tid == 0) sm.snap_out[(size_t)inst * sm.n_snap + snap.q] = snap_off >= 0 ? Ul[snap_off] : nan("");
            hadi_snap_advance(sm, snap);
        }
    }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    if (lane == 0)
        for (int k = 0; k < 12; k++) atomicAdd(&g_hadi_stamps[k], stamp_store_[k]);
#endif
    for (int e = tid; e < nrows * rowp; e += NT) Ug[e] = Ul[e];
    if constexpr (AMER) {
        double *__restrict__ Lg = a.LAM + (size_t)inst * a.L.inst_stride;
        for (int e = tid; e < nrows * rowp; e += NT) Lg[e] = LAMl[e];
    }
}

template <int B, int W, bool AMER>
__global__ void __launch_bounds__(64 * W) hadi_small_kernel(HadiSweepArgs a, HadiSmallArgs sm) {
    hadi_small_body<B, W, AMER, false>(a, sm);
}

// hadi_small_kernel<B, W, false> with the jump sub-step of a Bates call inside the time loop: a sampled Bates ladder is one launch.
// Its own symbol outside the table of hadi_dispatch.h (hadi_small_jump_fn), as hadi_small_sch_kernel is.
template <int B, int W>
__global__ void __launch_bounds__(64 * W) hadi_small_jump_kernel(HadiSweepArgs a, HadiSmallArgs sm) {
    hadi_small_body<B, W, false, true>(a, sm);
}

// ------------------------------------------------------------------------------------------------
// Small grids, European / dividend sweeps: ONE wavefront per instance, lines solved SEQUENTIALLY, one line per lane.
// The kernel above runs the big-grid row step on 51-node rows: a whole wavefront and six cyclic-reduction levels (54
// ds_bpermute, ~400 instructions) per row -- at one node per lane almost all of it is overhead, and 26 rows x 8
// wavefronts cost ~10 us per time step.  Here the roles are turned round, as in the reference's own team kernels
// (hes_a1_kernels.hpp:139-161, one thread per v-row; hes_a2_shuffled_kernels.hpp:243-299, one thread per s-column):
//   row pass     lane j <-> v-row j (nrows <= 33 lanes busy) walks i = 1 .. m1: explicit operators from a sliding window of
//                three columns (five new LDS values per node), Y0, forward Thomas with the pivot recomputed on the fly; the
//                back substitution walks i = m1 .. 1.  No cross-lane traffic at all.
//   column pass  lane i <-> s-column i: pentadiagonal forward / backward sweep with the precomputed factors.
// State in LDS in NATURAL order, pitch odd (conflict-free both ways): U (two zero halo rows above and below) and Y.  The
// forward sweep needs three values per node for the way back (the normalised right-hand side, the multiplier c', and the
// explicit A2 correction of the output) but only two arrays exist: the output is rewritten as
//   Y_i = x_i + corr_i = (ys_i + corr_i + c'_i corr_{i+1}) - c'_i Y_{i+1} = g_i - c'_i Y_{i+1},
// g_i goes to Y, and c'_i goes to column i-1 of U's own row -- every lane is at the same i (one wavefront), so that column
// has been consumed by all of them.  The column pass rebuilds U completely.  ~45 instructions per node against ~10 x that.
struct HadiSmallSeqLayout {
    int pitch;     // doubles per row in LDS: odd, >= m1 + 3 (columns m1 + 1, m1 + 2 stay zero: the s-neighbour of the last
                   // node and the column the one-ahead fetch touches behind it)
    int off_y, off_coef, off_b2, off_zero, off_dummy, off_ptab, total;  // offsets in doubles: U starts at 0 (nrows rows)
};
HADI_HD inline HadiSmallSeqLayout hadi_small_seq_layout(int m1, int nrows) {
    HadiSmallSeqLayout l;
    l.pitch = (m1 + 3) | 1;
    l.off_y = nrows * l.pitch;
    l.off_coef = l.off_y + nrows * l.pitch;
    l.off_coef = (l.off_coef + 1) & ~1;  // 16-byte aligned quads
    l.off_b2 = l.off_coef + 4 * (m1 + 2);
    l.off_zero = l.off_b2 + (m1 + 2);       // a row of zeros: the "b2 row" of every v-row but the last
    l.off_dummy = l.off_zero + (m1 + 2);    // where the idle lanes (>= nrows) put their results
    l.off_ptab = l.off_dummy + l.pitch;
    l.total = l.off_ptab + nrows * 5;
    return l;
}

template <int B>
__global__ void __launch_bounds__(64) hadi_small_seq_kernel(HadiSweepArgs a, HadiSmallArgs sm) {
    HADI_DYN_SMEM(double, smem);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.n_inst) return;
    const int inst = sm.order ? sm.order[blockIdx.x] : (int)blockIdx.x;
    const HadiInstPar ip = a.ipar[inst];
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1;
    const HadiSmallSeqLayout Ls = hadi_small_seq_layout(m1, nrows);
    const int PL = Ls.pitch;
    double *Ul = smem;  // row 0 of U
    double *Yl = smem + Ls.off_y;
    double *coefl = smem + Ls.off_coef;  // [i][4]: Bm, Bp, Dm, Dp of node i
    double *b2l = smem + Ls.off_b2;
    double *ptab = smem + Ls.off_ptab;   // [k][5]: L, L2, Q, C, C2

    for (int e = lane; e < Ls.total; e += 64) smem[e] = 0.0;
    __syncthreads();
    hadi_lds_stage_in<B>(smem, Ls, a, inst, lane);
    // this lane's v-row: its table entry stays in registers for the whole time loop
    const int j = lane;
    const bool act = j < nrows;
    const bool last = (j == nrows - 1);
    const HadiLdsRowTab tab = hadi_lds_row_table(a, inst, j, act);
    const double v = tab.v, wm = tab.wm, wz = tab.wz, wp = tab.wp, a2l2 = tab.a2l2, a2l1 = tab.a2l1, a2m = tab.a2m, a2u1 = tab.a2u1,
                 a2u2 = tab.a2u2, b1val = tab.b1val;
    const int b1col = tab.b1col;
    const bool b1_at0 = tab.b1_at0;
    const double dt = ip.dt, thdt = ip.thdt, qd = ip.q, half_rd = ip.half_rd;
    const double inv0 = 1.0 / (1.0 + ip.thdt * ip.hr0);
    const double *urow = Ul + (act ? j : 0) * PL;  // (idle lanes walk row 0 and store nothing)
    // The v-neighbours j-2 .. j+2, clamped to the grid instead of zero halo rows (1.7 KB that cost the sixth instance per CU):
    // a clamped row only ever meets a zero weight -- the first / last rows of A0 and A2 have no entries beyond the grid.
    // The v-neighbours j-2 .. j+2 of a column are the SAME column in the neighbouring LANES' rows: one LDS read of the own row
    // and four wave shifts (DPP) instead of five LDS reads per node -- at six wavefronts per CU the one LDS pipe, not the
    // SIMDs, is what this kernel fills (round 3).  Beyond the grid the shifts deliver 0 or an idle lane's (finite) value of
    // row 0; either only ever meets a zero weight -- the first / last rows of A0 and A2 have no entries beyond the grid.
    auto col5 = [&](const double own, double &m2v, double &m1v, double &p1v, double &p2v) {
        m1v = hadi_lane_prev(own); m2v = hadi_lane_prev(m1v);
        p1v = hadi_lane_next(own); p2v = hadi_lane_next(p1v);
    };
    double *yrow = act ? Yl + j * PL : smem + Ls.off_dummy;  // (idle lanes store into a dummy row)
    double *crow = act ? Ul + j * PL : smem + Ls.off_dummy;  // column i - 1 of this row receives c'_i
    const double *b2p = last ? b2l : smem + Ls.off_zero;      // b2 lives on the last v-row only
    __syncthreads();

    const int N = ip.N < sm.Nmax ? ip.N : sm.Nmax;
    HadiSnapCursor snap = hadi_snap_begin(sm);
    const int snap_off = sm.n_snap > 0 ? hadi_snap_natural(a.L, sm.snap_node[inst], PL) : -1;
    const double *__restrict__ vs = sm.vec_s ? sm.vec_s + (size_t)inst * (m1 + 1) : nullptr;
    for (int n = 1; n <= N; n++) {
        // ---- discrete dividend at the start of the step (device_solver.hpp:448-504) ---------------
        const int dv = sm.div_flag ? sm.div_flag[(size_t)inst * sm.flag_stride + n - 1] : -1;
        if (dv >= 0) {
            for (int e = lane; e < nrows * PL; e += 64) Yl[e] = Ul[e];  // U_temp
            __syncthreads();
            const double amount = sm.div_amounts[dv], pct = sm.div_pcts[dv];
            for (int e = lane; e < nrows * (m1 + 1); e += 64) {
                const int jj = e / (m1 + 1), i = e - jj * (m1 + 1);
                const double *src = Yl + jj * PL;
                Ul[jj * PL + i] =
                    hadi_dividend_jump(vs, m1, amount, pct, ip.put, i, [&](int k) { return src[k]; });
            }
            __syncthreads();
        }
        const double e_nm1 = exp(ip.bc_rate * ip.dt * (n - 1));  // device_solver.hpp:238
        const double e_n = exp(ip.bc_rate * ip.dt * n);          // device_solver.hpp:246
        const double cb1 = dt * e_nm1 + thdt * (e_n - e_nm1);
        const double b1l = b1val * cb1;
        // ---- row pass: lane <-> v-row, i = 1 .. m1 (same formulas as hadi_row_step) --------------------------------
        // Only the lanes that own a v-row run the sweeps: the LDS moves 16 or 8 bytes per ACTIVE lane, and with nrows of 64 lanes
        // busy that is less than half of what the idle lanes' dummy walk used to drag through the CU's one LDS pipe.  (The wave
        // shifts deliver 0 from a switched-off lane: the row beyond the last one only ever meets a zero weight.  The emulator's
        // lane threads all have to take part in its collective shuffles, so there every lane still runs.)
#if defined(HADI_EMU)
        const bool rowrun = true;
#else
        const bool rowrun = act;
#endif
        if (rowrun) {
#include "hadi_k_lds_row_body.h"
        }  // (rowrun)
        __syncthreads();
        // ---- column pass: lane <-> s-column ----
        hadi_lds_penta_cols(Yl, Ul, ptab, PL, nrows, m1, lane);
        __syncthreads();
        if (hadi_ex_listed(sm.ex_flag, sm.ex_stride, inst, n)) {  // Bermudan exercise at the end of the step (wave-uniform)
            hadi_exercise_lds<B>(Ul, PL, true, a.U0 + (size_t)inst * a.L.inst_stride, nrows, m1, rowp, lane, 64);
            __syncthreads();
        }
        if (hadi_ex_listed(sm.ko_flag, sm.ko_stride, inst, n)) {  // knock-out at the end of a monitoring step (wave-uniform)
            hadi_knock_lds<B>(Ul, PL, true, sm.ko_iab[2 * inst], sm.ko_iab[2 * inst + 1], sm.ko_rebate[inst], nrows, m1, lane, 64);
            __syncthreads();
        }
        if (hadi_ex_listed(sm.fix_flag, sm.fix_stride, inst, n)) {  // strike fixing behind the knock-out's place (wave-uniform)
            hadi_fixing_lds<B>(Ul, PL, true, a.U0 + (size_t)inst * a.L.inst_stride, sm.vec_s + (size_t)inst * (m1 + 1), sm.fix_iref[inst],
                               sm.fix_mode[inst], hadi_fix_weight(sm.fix_w, sm.fix_stride, inst, n), nrows, m1, rowp, lane, 64);
            __syncthreads();
        }
        // maturity ladder: lane 0 reads the node before it stores anything of the next step (one wavefront: nobody else has yet)
        if (n == snap.next) {
            if (sm.n_samp > 0) {  // sampled ladder: every lane reads before the row sweep of the next step parks c' in U
                hadi_sample_lds(sm, a.L, Ul, true, PL, inst, snap.q, lane, 64, true);
                __syncthreads();
            } else if (lane == 0) sm.snap_out[(size_t)inst * sm.n_snap + snap.q] = snap_off >= 0 ? Ul[snap_off] : nan("");
            hadi_snap_advance(sm, snap);
        }
    }
    hadi_lds_stage_out<B>(Ul, PL, a, inst, lane);
}

// ------------------------------------------------------------------------------------------------
// hadi_small_seq_kernel with TWO instances per wavefront (round 3).  The row sweep above keeps nrows of the 64 lanes busy
// -- 26 for the reference's 50x25 grid -- and is nine tenths of the kernel's instructions: here lanes 0..31 walk the v-rows
// of one instance and lanes 32..63 those of a second one through the SAME instruction stream (per-lane LDS base pointers
// and instance scalars; the wave shifts that fetch the v-neighbours meet zero weights across the boundary between the two
// instances exactly as they do beyond a grid's own first and last row).  The column sweeps (lane <-> s-column) run once
// per instance.  LDS: two instances' arrays per wavefront (52 KB for 50x25: three wavefronts = six instances per CU, as
// before), but a wavefront now retires two instances' time steps in little more than the time of one.  Instances with
// different numbers of time steps (multi-maturity batches, dispatched longest first) simply stop at their own N.
// Needs nrows <= 32.  The row sweep is the very text hadi_small_seq_kernel compiles (hadi_k_lds_row_body.h): the results are
// bit-identical.
template <int B>
__global__ void __launch_bounds__(64) hadi_small_seq2_kernel(HadiSweepArgs a, HadiSmallArgs sm) {
    HADI_DYN_SMEM(double, smem);
    const int lane = threadIdx.x;
    const int half = lane >> 5, jl = lane & 31;
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1;
    const HadiSmallSeqLayout Ls = hadi_small_seq_layout(m1, nrows);
    const int PL = Ls.pitch;
    // the two instances of this wavefront (the second slot of the last block may be empty)
    const int slot0 = 2 * (int)blockIdx.x, slot1 = slot0 + 1;
    if (slot0 >= a.n_inst) return;
    const bool has1 = slot1 < a.n_inst;
    const int inst0 = sm.order ? sm.order[slot0] : slot0;
    const int inst1 = has1 ? (sm.order ? sm.order[slot1] : slot1) : inst0;
    const int inst = half ? inst1 : inst0;             // this lane's instance
    const HadiInstPar ip = a.ipar[inst];               // (per lane: two different structs in the wavefront)
    const HadiInstPar ip0 = a.ipar[inst0], ip1 = a.ipar[inst1];
    const int N0 = ip0.N < sm.Nmax ? ip0.N : sm.Nmax;
    const int N1 = has1 ? (ip1.N < sm.Nmax ? ip1.N : sm.Nmax) : 0;
    const int Nw = N0 > N1 ? N0 : N1;                  // (wave-uniform)
    const int Nl = half ? N1 : N0;                     // this lane's number of time steps
    double *const base0 = smem, *const base1 = smem + Ls.total;
    double *const bl = half ? base1 : base0;           // this lane's instance in LDS
    double *Ul = bl;
    double *Yl = bl + Ls.off_y;
    double *coefl = bl + Ls.off_coef;                  // [i][4]: Bm, Bp, Dm, Dp of node i
    double *b2l = bl + Ls.off_b2;

    for (int e = lane; e < 2 * Ls.total; e += 64) smem[e] = 0.0;
    __syncthreads();
    for (int h = 0; h < (has1 ? 2 : 1); h++)           // (uniform loops: all 64 lanes copy one instance, then the other)
        hadi_lds_stage_in<B>(h ? base1 : base0, Ls, a, h ? inst1 : inst0, lane);
    // this lane's v-row of its instance: the table entry stays in registers for the whole time loop
    const int j = jl;
    const bool act = j < nrows && (half == 0 || has1);
    const bool last = (j == nrows - 1);
    const HadiLdsRowTab tab = hadi_lds_row_table(a, inst, j, act);
    const double v = tab.v, wm = tab.wm, wz = tab.wz, wp = tab.wp, a2l2 = tab.a2l2, a2l1 = tab.a2l1, a2m = tab.a2m, a2u1 = tab.a2u1,
                 a2u2 = tab.a2u2, b1val = tab.b1val;
    const int b1col = tab.b1col;
    const bool b1_at0 = tab.b1_at0;
    const double dt = ip.dt, thdt = ip.thdt, qd = ip.q, half_rd = ip.half_rd;
    const double inv0 = 1.0 / (1.0 + ip.thdt * ip.hr0);
    const double *urow = Ul + (act ? j : 0) * PL;  // (idle lanes walk row 0 and store nothing)
    auto col5 = [&](const double own, double &m2v, double &m1v, double &p1v, double &p2v) {
        m1v = hadi_lane_prev(own); m2v = hadi_lane_prev(m1v);
        p1v = hadi_lane_next(own); p2v = hadi_lane_next(p1v);
    };
    double *const yrow_real = act ? Yl + j * PL : bl + Ls.off_dummy;
    double *const crow_real = act ? Ul + j * PL : bl + Ls.off_dummy;
    const double *b2p = last ? b2l : bl + Ls.off_zero;      // b2 lives on the last v-row only
    __syncthreads();

    HadiSnapCursor snap = hadi_snap_begin(sm);
    // (lanes 0 and 32 serve the two instances; the odd last block has no second one)
    const int snap_off = (sm.n_snap > 0 && jl == 0 && (half == 0 || has1)) ? hadi_snap_natural(a.L, sm.snap_node[inst], PL) : -1;
    for (int n = 1; n <= Nw; n++) {
        // ---- discrete dividends at the start of the step, instance by instance (device_solver.hpp:448-504) ----
        for (int h = 0; h < (has1 ? 2 : 1); h++) {
            const int ih = h ? inst1 : inst0, Nh = h ? N1 : N0;
            const int dv = (sm.div_flag && n <= Nh) ? sm.div_flag[(size_t)ih * sm.flag_stride + n - 1] : -1;
            if (dv >= 0) {  // (wave-uniform)
                double *Uh = h ? base1 : base0, *Yh = Uh + Ls.off_y;
                const double *__restrict__ vs = sm.vec_s + (size_t)ih * (m1 + 1);
                const int put_h = h ? ip1.put : ip0.put;
                for (int e = lane; e < nrows * PL; e += 64) Yh[e] = Uh[e];  // U_temp
                __syncthreads();
                const double amount = sm.div_amounts[dv], pct = sm.div_pcts[dv];
                for (int e = lane; e < nrows * (m1 + 1); e += 64) {
                    const int jj = e / (m1 + 1), i = e - jj * (m1 + 1);
                    const double *src = Yh + jj * PL;
                    Uh[jj * PL + i] =
                        hadi_dividend_jump(vs, m1, amount, pct, put_h, i, [&](int k) { return src[k]; });
                }
                __syncthreads();
            }
        }
        const double e_nm1 = exp(ip.bc_rate * ip.dt * (n - 1));  // device_solver.hpp:238
        const double e_n = exp(ip.bc_rate * ip.dt * n);          // device_solver.hpp:246
        const double cb1 = dt * e_nm1 + thdt * (e_n - e_nm1);
        const double b1l = b1val * cb1;
        // a lane whose instance has finished its own N steps keeps walking (the wave shifts are collective) but stores into the
        // dummy row; on the GPU it is switched off altogether
        const bool live = act && n <= Nl;
        double *const yrow = live ? yrow_real : bl + Ls.off_dummy;
        double *const crow = live ? crow_real : bl + Ls.off_dummy;
#if defined(HADI_EMU)
        const bool rowrun = true;
#else
        const bool rowrun = live;
#endif
        if (rowrun) {
#include "hadi_k_lds_row_body.h"
        }  // (rowrun)
        __syncthreads();
        // ---- column pass, instance by instance: lane <-> s-column (hes_a2_shuffled_kernels.hpp:243-299) ----
        for (int h = 0; h < (has1 ? 2 : 1); h++) {
            if (n > (h ? N1 : N0)) continue;  // (wave-uniform)
            double *Uh = h ? base1 : base0, *Yh = Uh + Ls.off_y;
            const double *ptab = Uh + Ls.off_ptab;   // [k][5]: L, L2, Q, C, C2
            hadi_lds_penta_cols(Yh, Uh, ptab, PL, nrows, m1, lane);
        }
        __syncthreads();
        // Bermudan exercise at the end of the step, instance by instance: each on its own schedule and within its own N
        for (int h = 0; h < (has1 ? 2 : 1); h++) {
            const int ih = h ? inst1 : inst0, Nh = h ? N1 : N0;
            if (n <= Nh && hadi_ex_listed(sm.ex_flag, sm.ex_stride, ih, n)) {  // (wave-uniform)
                hadi_exercise_lds<B>(h ? base1 : base0, PL, true, a.U0 + (size_t)ih * a.L.inst_stride, nrows, m1, rowp, lane, 64);
                __syncthreads();
            }
            if (n <= Nh && hadi_ex_listed(sm.ko_flag, sm.ko_stride, ih, n)) {  // knock-out, per half as the exercise (wave-uniform)
                hadi_knock_lds<B>(h ? base1 : base0, PL, true, sm.ko_iab[2 * ih], sm.ko_iab[2 * ih + 1], sm.ko_rebate[ih], nrows, m1, lane, 64);
                __syncthreads();
            }
            if (n <= Nh && hadi_ex_listed(sm.fix_flag, sm.fix_stride, ih, n)) {  // strike fixing, per half as the knock-out (wave-uniform)
                hadi_fixing_lds<B>(h ? base1 : base0, PL, true, a.U0 + (size_t)ih * a.L.inst_stride, sm.vec_s + (size_t)ih * (m1 + 1),
                                   sm.fix_iref[ih], sm.fix_mode[ih], hadi_fix_weight(sm.fix_w, sm.fix_stride, ih, n), nrows, m1, rowp, lane, 64);
                __syncthreads();
            }
        }
        // maturity ladder: one lane per instance reads its node before it stores anything of the next step
        if (n == snap.next) {
            if (sm.n_samp > 0) {  // sampled ladder: the 32 lanes of a half take the samples of its instance
                hadi_sample_lds(sm, a.L, Ul, true, PL, inst, snap.q, jl, 32, (half == 0 || has1) && n <= Nl);
                __syncthreads();
            } else if (jl == 0 && (half == 0 || has1) && n <= Nl)
                sm.snap_out[(size_t)inst * sm.n_snap + snap.q] = snap_off >= 0 ? Ul[snap_off] : nan("");
            hadi_snap_advance(sm, snap);
        }
    }
    for (int h = 0; h < (has1 ? 2 : 1); h++) hadi_lds_stage_out<B>(h ? base1 : base0, PL, a, h ? inst1 : inst0, lane);
}

