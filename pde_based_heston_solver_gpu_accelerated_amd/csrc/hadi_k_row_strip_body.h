// hadi_k_row_strip_body.h -- the body of the strip row-pass kernels hadi_pass_a_strip and hadi_pass_a_strip_sch
// (hadi_k_row_strip.h), included inside both.  Template parameters in scope: B, AMER, T, G, MODE, SCH.  No include guard.
    static_assert(sizeof(T) == 8 || AMER == 0, "the fp32-state sweep is European only");
    static_assert(G == 1 || (G == 2 && B == 8), "paired strips: 8 nodes per lane");
    static_assert(MODE == 0 || (AMER == 0 && sizeof(T) == 8), "Craig-Sneyd: European sweeps, fp64 state");
    static_assert(MODE != 3 || G == 2, "MODE 3: the coupling-column table of the paired strips");
    // paired strips: the pair's coupling column from the table MODE 3 built at the start of the solve (hadi_strip_step, RSTAB)
#ifndef HADI_PAIR_RSTAB
#define HADI_PAIR_RSTAB 1
#endif
    // (not the P representation: that kernel sits at 256 VGPRs, and the two registers the table entry keeps across the step
    // sent six others to scratch -- a scratch reload inside the row loop drains the DMA prefetch)
    // ... and not the explicit (U, lambda_bar) pair either: measured 3 % SLOWER there (its lambda_bar rows are register loads of the
    // compiler already; one more shifts its waits) -- European sweeps, both state precisions (profiles/r04_pair_spike_ab.txt)
    constexpr bool RSTAB = (G == 2 && MODE == 0 && AMER == 0 && HADI_PAIR_RSTAB);
    HADI_DYN_SMEM(double, smem);
    constexpr int NS = HADI_STRIP_NS(B, G, (int)sizeof(T)), NWV = HADI_STRIP_WAVES(B), NPAIR = NWV / G, c0slot = 64 * B * G;
    // American P representation at 8 nodes per lane: one slot stays BEHIND the prefetch -- row j itself, whose raw P the step
    // reads again for lambda_bar -- so the row D = NS - 1 ahead is fetched, not the row NS ahead
    constexpr int KEEP = (AMER == 2 && B >= HADI_AMP_KEEP_MIN_B && G == 1) ? 1 : 0, D = NS - KEEP;
    constexpr int NA = D - 2;  // DMA batches in flight behind the one that is waited for
    const int lane = threadIdx.x & 63;
    const int wave = HADI_UNIFORM((int)(threadIdx.x >> 6));
    const int pair = wave / G, half = wave - pair * G;  // (G = 1: pair = wave, half = 0)
    const int total = a.n_inst * a.sblocks;
    const int logical = hadi_xcd_remap(blockIdx.x, gridDim.x);
    if (logical >= total) return;
    const int inst = logical / a.sblocks, sb = logical - inst * a.sblocks;
    // The instance's parameter block is REQUESTED here and CONSUMED behind the prologue's row fetches (round 4): consumed at
    // once -- `if (n > ip.N) return` -- its memory round trip (1 - 2 us, one per launch and wavefront, nothing to overlap it
    // with) stood in front of every other load of the prologue; a launch of short strips is mostly prologue.
    const HadiInstPar ip = a.ipar[inst];
    const int nrows = a.L.nrows, npad = a.L.nrows_pad, rowp = a.L.rowp;
    double *coef = reinterpret_cast<double *>(reinterpret_cast<T *>(smem) + (size_t)NPAIR * NS * rowp);
    // P representation: the payoff row (it depends on s only: v-row 0 of the packed payoff) behind the coefficient arrays;
    // re-read from LDS every row rather than held in 2 B registers per lane (that version spilled)
    const double *payl = coef + 4 * 64 * B * G;
    const int j0 = (sb * NPAIR + pair) * a.RS;
    const bool has_strip = j0 < nrows;  // (wave-uniform; a wavefront without a strip only helps with the shared copies below)
    const int j1 = (j0 + a.RS < nrows) ? j0 + a.RS : nrows;

    HadiStripCtxT<T> c;
    c.lane = lane;
    c.rowp = rowp;
    c.coef = coef;
    c.half = half;
    double *const xch0 = coef + 4 * 64 * B * G + (AMER == 2 ? rowp : 0);  // the pairs' exchange buffers (behind the payoff row)
    c.xch = xch0 + pair * 16;
    c.err = a.err; c.debug = a.debug;
    const T *__restrict__ Ub = reinterpret_cast<const T *>(a.U) + (size_t)inst * a.L.inst_stride;
    c.Yi = reinterpret_cast<T *>(a.Y) + (size_t)inst * a.L.inst_stride;
    c.Li = (AMER == 1) ? a.LAM + (size_t)inst * a.L.inst_stride : nullptr;
    c.R1i = MODE ? a.R1 + (size_t)inst * a.L.inst_stride : nullptr;
    c.C2i = MODE ? a.C2 + (size_t)inst * a.L.inst_stride : nullptr;
    c.b2r = a.b2row + (size_t)inst * rowp;
    // P representation: 1/dt, and which node is s_max (lambda_bar stays 0 there, as in hadi_row_step)
    c.inv_dt = 0.0; c.m1_lane = -1; c.m1_r = -1;
    if constexpr (AMER == 2) {
        const int e1 = a.L.m1 - 1;  // node i = m1 is element m1 - 1 of the row's 64 B G interior nodes
        if (e1 / (64 * B) == half) {
            c.m1_lane = (e1 - half * 64 * B) / B;
            c.m1_r = (e1 - half * 64 * B) % B;
        }
    }

    T *ring = reinterpret_cast<T *>(smem) + (size_t)pair * NS * rowp;
    auto slot = [&](int jj) { return ring + (size_t)((NS & (NS - 1)) == 0 ? (jj & (NS - 1)) : (jj + 12) % NS) * rowp; };  // (jj >= -4)
    // returns the number of vector-memory instructions issued (rows outside the allocation are zero-filled)
    auto fetch = [&](int jj) -> int {
        const bool exists = jj >= 0 && jj < npad;
        if constexpr (G > 1) {
            return hadi_half_row_to_lds<B, T>(Ub + (ptrdiff_t)jj * rowp, slot(jj), half, lane, exists);
        } else {
            hadi_row_to_lds_fixed<B, T>(Ub + (ptrdiff_t)jj * rowp, slot(jj), lane, exists);
            return exists ? hadi_row_dma_count<T>(rowp) : 0;
        }
    };
    // Direction of the walk: even strips go up (j0 -> j1-1), odd strips come down (j1-1 -> j0).  Neighbouring strips
    // then touch their shared halo rows at the same time -- both start there or both end there -- so the second reader
    // finds them in L2 instead of fetching them again ~100 us later (HBM reads of this pass 9.8 -> ~9 B per node).
    // Below, "behind" = rows already passed (registers), "ahead" = rows still to come (LDS ring / in flight); for a
    // descending strip the row-table scalars of the +1/+2 and -1/-2 neighbours simply swap roles.
    // Round 4: EVEN strips come down, ODD strips go up, so the strips 2k and 2k+1 -- always in the same block -- START on
    // either side of their common boundary.  What one of them has behind it at the start (two rows) is what the other starts
    // on and has one ahead: those rows are read from the partner's ring after the prologue's barrier instead of from memory a
    // second time, and the strip's own first row comes through its ring as well (`shared` below): cnt + 2 rows per strip by
    // LDS-DMA and nothing else, where cnt + 1 + 3 were read.
    const int sidx = sb * NPAIR + pair;
    const int dir = (sidx & 1) ? 1 : -1;
    const int cnt = j1 - j0;
    const int js = dir > 0 ? j0 : j1 - 1;
    auto row_ok = [&](int jj) { return jj >= 0 && jj < npad; };
    // (wave-uniform) the partner strip exists; a last strip without one keeps the register loads of its rows behind
    const bool shared = has_strip && (sidx ^ 1) * a.RS < nrows;
    const T *pring = reinterpret_cast<T *>(smem) + (size_t)(pair ^ 1) * NS * rowp;
    auto pslot = [&](int jj) { return pring + (size_t)((NS & (NS - 1)) == 0 ? (jj & (NS - 1)) : (jj + 12) % NS) * rowp; };
    // ---- prologue: the next rows ahead to the ring, the two rows behind and the first row to registers ----
    // aft[k] = vector-memory instructions issued after the DMA of the row 2 + k ahead: aft[0] belongs to the row that is
    // waited for next, the row NS - 1 ahead is the youngest DMA (nothing behind it yet)
    int aft[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) aft[k] = 0;
    // Order of the prologue: this wavefront's row fetches (LDS-DMA) and register loads are ISSUED first, then the block
    // copies the shared s-coefficient arrays (global -> LDS) and meets at the only block-wide barrier -- the two memory
    // round trips overlap instead of following each other (a launch of short strips is mostly prologue: 64 instances of
    // 512x256, 9-row strips: 0.0380 -> see DESIGN.md section 5).
    if (has_strip) {
        if (KEEP || shared) fetch(js);  // (the first row too: the step reads its raw P from the ring / `shared` above)
        fetch(js + dir);
        fetch(js + 2 * dir);
#pragma unroll
        for (int q = 3; q < D; q++) {
            const int zq = fetch(js + q * dir);
#pragma unroll
            for (int k = 0; k < NA; k++)
                if (k + 2 < q) aft[k] += zq;
        }
    }
    double rs_next = 0.0;  // RSTAB: the table entry of the NEXT step's row (an ordinary load, requested a step ahead: hadi_cs_row_load)
    const double *rs_lane = (RSTAB || MODE == 3) ? a.rs_tab + ((size_t)inst * nrows * 2 + half) * 64 + lane : nullptr;  // + 128 j
    if constexpr (RSTAB) rs_next = hadi_nt_load(rs_lane + (size_t)(has_strip ? js : 0) * 128);
    HadiCsRow<B> cs_next;  // MODE 2: R1 / C2 of the NEXT step's row (requested a step ahead)
    if constexpr (MODE == 2) {
        const size_t ro = (size_t)(has_strip ? js : 0) * rowp;
        hadi_cs_row_load<B, G>(c.R1i + ro, c.C2i + ro, half, lane, cs_next);
    }
    // rows behind by 2, behind by 1 (carried in the state's own type: with an fp32 state they are exact floats and cost
    // half the registers), current row (double: used throughout the step)
    T um2[B], um1[B];
    double u0[B];
    // The i = 0 column of the five stencil rows is wave-uniform: ONE register pair carries it, spread over the lanes
    // (lane k = row j - 2 + k in walking order), read with v_readlane where needed and shifted by a DPP move per step.
    // G = 2: the low half owns the i = 0 column; `evec` carries, the same way, the partner's node next to this half (the
    // high half's first node for the low half and vice versa) on the rows behind / at / ahead of j (lanes 1, 2, 3).
    double c0vec, evec = 0.0;
    int epos = 0;
    if constexpr (G > 1) {
        const int inode = (half == 0) ? 64 * B + 1 : 64 * B;
        epos = (sizeof(T) == 4) ? hadi_pos_f32(B, G, inode) : hadi_pos(B, G, inode);
    }
    double t2[B], t1[B];
#pragma unroll
    for (int r = 0; r < B; r++) t2[r] = t1[r] = u0[r] = 0.0;
    c0vec = 0.0;
    if (has_strip) {
        if (!shared) {
            if (row_ok(js - 2 * dir)) hadi_get_block<B, G, T>(Ub + (ptrdiff_t)(js - 2 * dir) * rowp, half, lane, t2);
            if (row_ok(js - dir)) hadi_get_block<B, G, T>(Ub + (ptrdiff_t)(js - dir) * rowp, half, lane, t1);
            hadi_get_block<B, G, T>(Ub + (size_t)js * rowp, half, lane, u0);
        }
        const int rr = js + (lane - 2) * dir;
        c0vec = (half == 0 && lane < 4 && row_ok(rr)) ? (double)Ub[(ptrdiff_t)rr * rowp + c0slot] : 0.0;
        if constexpr (G > 1) evec = (lane < 4 && row_ok(rr)) ? (double)Ub[(ptrdiff_t)rr * rowp + epos] : 0.0;
    }
    // the shared arrays' global loads are issued before the parameter block is consumed as well: the scaling by it and the
    // LDS stores follow below (two dependent memory round trips of the prologue become one)
    constexpr int NCOPY = (4 * 64 * B * G) / (64 * NWV);
    static_assert(NCOPY * 64 * NWV == 4 * 64 * B * G, "coefficient arrays: whole rounds of the block");
    // Resident sweep (HADI_BODY_RESTAGE, set by hadi_resident_row_phase alone): the arrays do not depend on the step and nothing
    // aliases them between two row phases of a launch, so only the block's first step loads, scales and stores them.
#if defined(HADI_BODY_RESTAGE)
    const bool restage = (HADI_BODY_RESTAGE);  // (block-uniform)
#else
    constexpr bool restage = true;
#endif
    double sc_tmp[NCOPY];
#if defined(HADI_BODY_RESTAGE)
#pragma unroll
    for (int q = 0; q < NCOPY; q++) sc_tmp[q] = 0.0;
#endif
    if (restage) {
        const double *__restrict__ sc = a.scoef + (size_t)inst * 4 * 64 * B * G;
#pragma unroll
        for (int q = 0; q < NCOPY; q++) sc_tmp[q] = sc[threadIdx.x + q * 64 * NWV];
    }
    // ---- the instance's parameters are consumed here, behind the row fetches (see the top) ----
    if (n > ip.N) {  // (block-uniform: this instance has fewer time steps -- multi-maturity batches)
#if !defined(HADI_EMU)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA of this wavefront may outlive it
#endif
        return;
    }
    c.dt = hadi_uniform_d(ip.dt); c.thdt = hadi_uniform_d(ip.thdt);
    hadi_strip_theta(c, ip);
    c.hr0 = hadi_uniform_d(ip.hr0); c.inv0 = hadi_uniform_d(1.0 / (1.0 + ip.thdt * ip.hr0));
    c.e_nm1 = hadi_uniform_d(exp(ip.bc_rate * ip.dt * (n - 1)));  // device_solver.hpp:238
    c.e_n = hadi_uniform_d(exp(ip.bc_rate * ip.dt * n));          // device_solver.hpp:246
    if constexpr (AMER == 2) c.inv_dt = hadi_uniform_d(1.0 / ip.dt);
    if (restage) {  // s-coefficient arrays to LDS; the two beta arrays scaled by -theta dt (r_d - r_f) on the way (hadi_strip_step)
        const double mq = -(ip.thdt * ip.q);
#pragma unroll
        for (int q = 0; q < NCOPY; q++) {
            const int e = threadIdx.x + q * 64 * NWV;
            coef[e] = (e < 2 * 64 * B * G) ? mq * sc_tmp[q] : sc_tmp[q];
        }
    }
    if constexpr (AMER == 2) {
        const double *__restrict__ pg = a.U0 + (size_t)inst * a.L.inst_stride;
        double *pw = coef + 4 * 64 * B * G;
        for (int e = threadIdx.x; e < rowp; e += 64 * NWV) pw[e] = pg[e];
    }
    if constexpr (G > 1) {  // the pairs' exchange buffers (values + rendezvous tokens, all zero: no row has token 0)
        if (threadIdx.x < NPAIR * 16) xch0[threadIdx.x] = 0.0;
    }
    hadi_wait_vmcnt(0);  // this wavefront's prologue rows have landed (the partner reads two of them behind the barrier)
    __syncthreads();     // the coefficient arrays are shared
    if (shared) {
        hadi_get_block<B, G, T>(pslot(js - 2 * dir), half, lane, t2);  // = the partner's row one ahead
        hadi_get_block<B, G, T>(pslot(js - dir), half, lane, t1);      // = the partner's first row
        hadi_get_block<B, G, T>(slot(js), half, lane, u0);
#if !defined(HADI_EMU)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    }
    __syncthreads();  // ... and nobody's first fetch of the loop lands in a slot its partner is still reading
#if defined(HADI_BODY_RESTAGE)
    HADI_RES_STAMP(0);  // row prologue
#endif
    if (!has_strip) return;
    // 8 nodes per lane, European fp64 (the headline kernel): two of the four arrays fit the registers left over (224 -> 250
    // VGPRs, no spill): 8 of the 16 coefficient reads per row step less on the LDS pipe, +0.7 % on 512x256 x256 (three
    // interleaved runs of each build on one box, gpurun_out/r03aa); 3: only the last array (no gain measured)
#ifndef HADI_STRIP_CREG8
#define HADI_STRIP_CREG8 2
#endif
    constexpr int CREG = (B <= HADI_STRIP_CREG_MAX_B && G == 1) ? 1 : (B == 8 && G == 1 && AMER == 0 && sizeof(T) == 8 && MODE == 0) ? HADI_STRIP_CREG8 : 0;
    double cf[4 * B];
    if constexpr (CREG) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double t[B];
            hadi_get_block<B, 1>(coef + q * 64 * B, 0, lane, t);
#pragma unroll
            for (int r = 0; r < B; r++) cf[q * B + r] = t[r];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4 * B; e++) cf[e] = 0.0;
    }
    if constexpr (AMER == 2) {  // U = max(P, U_0) on the rows behind (the current row keeps its raw P for lambda_bar)
        double pay[B];
        hadi_get_block<B, G>(payl, half, lane, pay);
#pragma unroll
        for (int r = 0; r < B; r++) {
            t2[r] = fmax(t2[r], pay[r]);
            t1[r] = fmax(t1[r], pay[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < B; r++) {
        um2[r] = (T)t2[r];
        um1[r] = (T)t1[r];
    }
#if !defined(HADI_EMU)
    // Consume the prologue's register loads HERE: otherwise hipcc parks their s_waitcnt vmcnt(0) at the loop header,
    // where it would retire the DMA prefetch and the result stores in every iteration.
#pragma unroll
    for (int r = 0; r < B; r++) asm volatile("" : "+v"(um2[r]), "+v"(um1[r]), "+v"(u0[r]));  // (T and double operands)
    asm volatile("" : "+v"(c0vec));
    if constexpr (G > 1) asm volatile("" : "+v"(evec));
#endif

#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    unsigned long long stamp_store_[32] = {0};
    c.stamp_acc_ = stamp_store_;
#endif
    HADI_STAMP_DECL(c.stamp_acc_)
    for (int t = 0; t < cnt; t++) {
        const int j = js + dir * t;
        HADI_STAMPC(30);  // carry + loop
        HadiSRow srow;
        // (round 4, measured and dropped: requesting the entry one step AHEAD -- at the end of the step before, the first one in
        // the prologue -- keeps 24 scalar registers live across the loop edge; at 106 SGPRs the compiler parks them in VGPR
        // lanes (two variants even spill to scratch): row pass +1.2 % at 33-row strips, +3 % at 9 rows, +6.5 % on paired strips)
        hadi_sload_issue(a.rowc + ((size_t)inst * nrows + j) * HADI_RC + HADI_SRC0, srow);  // flies during the DMA wait
        double rs_cur = 0.0;
        if constexpr (RSTAB) {
            rs_cur = rs_next;  // (the compiler's wait for the load of a step ago sits here, in front of this step's loads and DMA)
            int nl = 0;
#if !defined(HADI_EMU)
            asm volatile("" : "+v"(rs_cur) :: "memory");
#endif
            if (t + 1 < cnt) {
                rs_next = hadi_nt_load(rs_lane + (size_t)(j + dir) * 128);  // (non-temporal: 33 MB of table per step must not displace Y from the memory-side cache -- the column pass ran 4 % slower with default-policy loads here)
                nl = 1;
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");
#endif
#pragma unroll
            for (int k = 0; k < NA; k++) aft[k] += nl;
        }
        HadiCsRow<B> csrow;
        if constexpr (MODE == 2) {
            csrow = cs_next;  // (the compiler's own wait for the loads of a step ago sits in front of their first use)
            int nl = 0;
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");  // the next row's loads stay HERE: behind the stores of the step before, ahead of this step's DMA
#endif
            if (t + 1 < cnt) {
                const size_t ro = (size_t)(j + dir) * rowp;
                nl = hadi_cs_row_load<B, G>(c.R1i + ro, c.C2i + ro, half, lane, cs_next);
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");
#endif
#pragma unroll
            for (int k = 0; k < NA; k++) aft[k] += nl;  // (they come behind every DMA batch in flight)
        }
        hadi_wave_rendezvous();
        // the row D ahead goes to the slot of row j (of row j - 1 when one slot is kept behind): that row is in registers,
        // and this wavefront's last read of the slot (in the previous step) has been retired there.  Issued BEFORE the
        // wait below, so that the prefetch does not queue behind it.
        int z = 0;
        if (t + D <= cnt + 1) z = fetch(j + D * dir);
        hadi_wait_vmcnt(aft[0] + z);  // the row two ahead has landed (the row one ahead landed a step earlier)
        HADI_STAMPC(24);  // wait for the DMA
#pragma unroll
        for (int k = 0; k + 1 < NA; k++) aft[k] = aft[k + 1] + z;
        aft[NA - 1] = 0;
        hadi_wave_rendezvous();
        double up1[B], up2[B];
        hadi_get_block<B, G, T>(slot(j + dir), half, lane, up1);
        hadi_get_block<B, G, T>(slot(j + 2 * dir), half, lane, up2);
        if (half == 0) {  // (wave-uniform; always true for G = 1)
            const double c0new = (double)slot(j + 2 * dir)[c0slot];  // (every lane reads the same word)
            c0vec = (lane == 4) ? c0new : c0vec;
        }
        double rt[HADI_RCL];
        hadi_sload_wait(srow, rt);  // one lgkmcnt(0) for the table entry and the LDS reads above
        if (dir < 0) {  // descending: "behind" rows are j+1, j+2 -- swap the neighbour weights instead of the arrays
            double w;
            w = rt[RC_WMS - HADI_SRC0]; rt[RC_WMS - HADI_SRC0] = rt[RC_WPS - HADI_SRC0]; rt[RC_WPS - HADI_SRC0] = w;
            w = rt[RC_L2 - HADI_SRC0]; rt[RC_L2 - HADI_SRC0] = rt[RC_U2 - HADI_SRC0]; rt[RC_U2 - HADI_SRC0] = w;
            w = rt[RC_L1 - HADI_SRC0]; rt[RC_L1 - HADI_SRC0] = rt[RC_U1 - HADI_SRC0]; rt[RC_U1 - HADI_SRC0] = w;
        }
        HADI_STAMPC(25);  // LDS reads + table entry + DMA issue
        double praw[B], lamc0 = 0.0;
        const double c0m2 = hadi_read_lane(c0vec, 0), c0m1 = hadi_read_lane(c0vec, 1), c00 = hadi_read_lane(c0vec, 2);
        const double c0p1 = hadi_read_lane(c0vec, 3), c0p2 = hadi_read_lane(c0vec, 4);
        double e0m2 = c0m2, e0m1 = c0m1, e00 = c00, e0p1 = c0p1, e0p2 = c0p2;  // (the carried i = 0 values stay raw)
#pragma unroll
        for (int r = 0; r < B; r++) praw[r] = 0.0;
        if constexpr (AMER == 2) {
            double pay[B];
            hadi_get_block<B, G>(payl, half, lane, pay);
            const double pay_c0 = payl[c0slot];
#pragma unroll
            for (int r = 0; r < B; r++) {
                if constexpr (G == 2) {
                    // paired strips: u0 stays the raw P (hadi_strip_step, RAW_U0); the row behind was carried raw as well
                    um1[r] = (T)fmax((double)um1[r], pay[r]);
                } else {
                    if constexpr (!KEEP) praw[r] = u0[r];  // the raw P of row j: lambda_bar comes from it inside the step
                    u0[r] = fmax(u0[r], pay[r]);
                }
                up1[r] = fmax(up1[r], pay[r]);
                up2[r] = fmax(up2[r], pay[r]);
            }
            lamc0 = fmax(0.0, (pay_c0 - c00) * c.inv_dt);
            e0m2 = fmax(c0m2, pay_c0); e0m1 = fmax(c0m1, pay_c0); e00 = fmax(c00, pay_c0);
            e0p1 = fmax(c0p1, pay_c0); e0p2 = fmax(c0p2, pay_c0);
        }
        double dm2[B], dm1[B];
#pragma unroll
        for (int r = 0; r < B; r++) {
            dm2[r] = (double)um2[r];
            dm1[r] = (double)um1[r];
        }
        double un[B];
        double xb_ = 0.0, x0_ = 0.0, xa_ = 0.0;  // the partner's boundary node on the rows behind / at / ahead (G = 2)
        if constexpr (G > 1) {
            xb_ = hadi_read_lane(evec, 1); x0_ = hadi_read_lane(evec, 2); xa_ = hadi_read_lane(evec, 3);
            if constexpr (AMER == 2) {  // (the carried values stay raw P: U = max(P, U_0) on the partner's node too)
                const double pay_e = payl[epos];
                xb_ = fmax(xb_, pay_e); x0_ = fmax(x0_, pay_e); xa_ = fmax(xa_, pay_e);
            }
        }
        double *rs_out = (MODE == 3) ? const_cast<double *>(rs_lane) + (size_t)j * 128 : nullptr;
        if (MODE < 2 && j == nrows - 1) hadi_strip_step<B, AMER, (MODE < 2), T, G, CREG, MODE, RSTAB, SCH>(c, j, rt, dm2, dm1, u0, up1, up2, e0m2, e0m1, e00, e0p1, e0p2, praw, lamc0, slot(j + dir), un, xb_, x0_, xa_, slot(j), payl, cf, &csrow, rs_cur, rs_out);
        else hadi_strip_step<B, AMER, false, T, G, CREG, MODE, RSTAB, SCH>(c, j, rt, dm2, dm1, u0, up1, up2, e0m2, e0m1, e00, e0p1, e0p2, praw, lamc0, slot(j + dir), un, xb_, x0_, xa_, slot(j), payl, cf, &csrow, rs_cur, rs_out);
        // the row's vector stores (the i = 0 stores are not counted: lower bound); the predictor stores R1 and C2 as well; the
        // table build (MODE 3) stores one double per lane (counted as nothing: lower bound)
        constexpr int NST = (MODE == 3 ? 0 : MODE == 1 ? 3 : 1) * hadi_put_block_stores<B, T>();
#pragma unroll
        for (int k = 0; k < NA; k++) aft[k] += NST;
        double enew = 0.0;
        if constexpr (G > 1) {
            // The partner's boundary node of the row TWO ahead, from the partner's half of the ring slot.  Safe here and only
            // here: the partner retired its DMA of that row before it published this step's token (which the exchange inside
            // the step has just seen), and it refills that slot two steps on -- after the next exchange, which needs this
            // wavefront's next token.
            enew = (double)slot(j + 2 * dir)[epos];  // (every lane reads the same word)
        }
#pragma unroll
        for (int r = 0; r < B; r++) {
            um2[r] = um1[r];
            um1[r] = (T)u0[r];
            u0[r] = un[r];
        }
#if !defined(HADI_EMU)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the re-read is retired before the next step reuses that slot
#endif
        c0vec = hadi_lane_next(c0vec);  // lane k takes lane k + 1: one row on
        if constexpr (G > 1) {
            evec = hadi_lane_next(evec);
            evec = (lane == 3) ? enew : evec;
        }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev_) :: "memory");  // the step stamped itself
#endif
    }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    if (HADI_STAMPS == 4 && lane == 0)
        for (int k = 24; k < 31; k++) atomicAdd(&g_hadi_stamps[k], stamp_store_[k]);
#endif
