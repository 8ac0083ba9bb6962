// hadi_k_row_ring_body.h -- the body of the shared-ring row-pass kernels hadi_pass_a and hadi_pass_a_sch (hadi_k_row_ring.h),
// included inside both.  Template parameters in scope: B, G, W, NG, PD, AMER, MODE, T, SCH.  No include guard.
    static_assert(sizeof(T) == 8 || (!AMER && MODE == 0), "the fp32-state sweep covers the European Douglas step only");
    HADI_DYN_SMEM(double, smem);
    constexpr int RING = (PD + 1) * W + 4;
    constexpr int NT = 64 * W * G * NG;
    const int lane = threadIdx.x & 63;
    const int wave = HADI_UNIFORM((int)(threadIdx.x >> 6));
    const int grp = wave / (W * G), wv = wave - grp * (W * G);
    const int wrow = wv / G, half = wv - wrow * G;
    const int tblocks = (a.ntiles + NG - 1) / NG;  // blocks per instance
    const int total = a.n_inst * tblocks;
    const int logical = hadi_xcd_remap(blockIdx.x, gridDim.x);
    if (logical >= total) return;
    const int inst = logical / tblocks, tb = logical - inst * tblocks;
    const HadiInstPar ip = a.ipar[inst];
    if (n > ip.N) return;
    const int nrows = a.L.nrows, npad = a.L.nrows_pad, rowp = a.L.rowp;
    const int tile = tb * NG + grp;
    const int j0 = tile * a.R;  // may be >= nrows for the last block's spare group: that group only joins barriers
    const int j1 = (j0 + a.R < nrows) ? j0 + a.R : nrows;

    HadiRowCtxT<T> c;
    c.lane = lane;
    c.half = half;
    c.wrow = wrow;
    c.rowp = rowp;
    c.dt = ip.dt; c.thdt = ip.thdt; c.qd = ip.q; c.half_rd = ip.half_rd;
    c.hr0 = ip.hr0; c.inv0 = 1.0 / (1.0 + ip.thdt * ip.hr0);
    if constexpr (SCH != HADI_SCH_CS) {
        c.ka = hadi_sch_ka(ip.dt, ip.thdt); c.kb = hadi_sch_kb<SCH>(ip.dt, ip.thdt);
        c.kc = hadi_sch_kc<SCH>(ip.dt, ip.thdt); c.kt = hadi_sch_kt<SCH>(ip.dt, ip.thdt);
    }
    c.e_nm1 = exp(ip.bc_rate * ip.dt * (n - 1));  // device_solver.hpp:238
    c.e_n = exp(ip.bc_rate * ip.dt * n);          // device_solver.hpp:246
    const T *__restrict__ Ub = reinterpret_cast<const T *>(a.U) + (size_t)inst * a.L.inst_stride;
    c.Yi = reinterpret_cast<T *>(a.Y) + (size_t)inst * a.L.inst_stride;
    c.Li = (AMER == 1) ? a.LAM + (size_t)inst * a.L.inst_stride : nullptr;
    c.b2r = a.b2row + (size_t)inst * rowp;
    c.R1i = MODE ? a.R1 + (size_t)inst * a.L.inst_stride : nullptr;
    c.C2i = MODE ? a.C2 + (size_t)inst * a.L.inst_stride : nullptr;
    c.j0 = j0;
    c.err = a.err; c.debug = a.debug;
    constexpr int c0slot = 64 * B * G;
    // storage positions of the s-neighbours of this lane's block (node before its first, node after its
    // last).  Before i = 1 comes the i = 0 slot; after the row's last node comes a pad slot (always 0).
    {
        const int ifirst = 1 + 64 * B * half + B * lane;
        if constexpr (sizeof(T) == 4) {
            c.posL = hadi_pos_f32(B, G, ifirst - 1);
            c.posR = (ifirst + B <= 64 * B * G) ? hadi_pos_f32(B, G, ifirst + B) : c0slot + 1;
        } else {
            c.posL = hadi_pos(B, G, ifirst - 1);
            c.posR = (ifirst + B <= 64 * B * G) ? hadi_pos(B, G, ifirst + B) : c0slot + 1;
        }
    }

    // LDS: [NG rings of RING rows of T] [4 coefficient arrays of 64*B*G] [NG*W*8 exchange] [NG compact row tables]
    T *ring = reinterpret_cast<T *>(smem) + (size_t)grp * RING * rowp;
    double *coef = reinterpret_cast<double *>(reinterpret_cast<T *>(smem) + (size_t)NG * RING * rowp);
    {
        const double *__restrict__ sc = a.scoef + (size_t)inst * 4 * 64 * B * G;
        for (int e = threadIdx.x; e < 4 * 64 * B * G; e += NT) coef[e] = sc[e];
    }
    c.coef = coef;
    c.xch = coef + 4 * 64 * B * G + grp * 8 * W;  // per v-row: 4 exchange values + the two rendezvous tokens
    if (threadIdx.x < 8 * W * NG) coef[4 * 64 * B * G + threadIdx.x] = 0.0;  // (tokens start at 0; the first loop barrier publishes this)
    {
        double *rtab = coef + 4 * 64 * B * G + NG * 8 * W + (size_t)grp * a.R * HADI_RCL;
        const double *__restrict__ rg = a.rowc + ((size_t)inst * nrows + j0) * HADI_RC;
        const int tl = threadIdx.x - grp * 64 * W * G;
        for (int e = tl; e < (j1 - j0) * HADI_RCL; e += 64 * W * G) rtab[e] = rg[(e / HADI_RCL) * HADI_RC + e % HADI_RCL];
        c.rowc = rtab;
        c.payrow = nullptr; c.inv_dt = 0.0; c.m1_lane = -1; c.m1_r = -1;
        if constexpr (AMER == 2) {  // payoff row (v-row 0 of the packed payoff; it depends on s only) after the tables
            double *prow = coef + 4 * 64 * B * G + NG * 8 * W + (size_t)NG * a.R * HADI_RCL;
            const double *__restrict__ pg = a.U0 + (size_t)inst * a.L.inst_stride;
            for (int e = threadIdx.x; e < rowp; e += NT) prow[e] = pg[e];
            c.payrow = prow;
            c.inv_dt = 1.0 / ip.dt;
            const int e1 = a.L.m1 - 1;  // node i = m1 is element m1-1 of the row's 64*B*G interior nodes
            if (e1 / (64 * B) == half) {
                c.m1_lane = (e1 - half * 64 * B) / B;
                c.m1_r = (e1 - half * 64 * B) % B;
            }
        }
    }

    const int iters = (j1 > j0) ? (j1 - j0 + W - 1) / W : 0;  // this group's iterations
    const int iters_all = (a.R + W - 1) / W;                   // every group of the block runs this many barriers
    auto slot = [&](int jj) { return ring + (size_t)((jj + 4 * RING) % RING) * rowp; };
    // fetch returns the number of vector-memory instructions it issued
    auto fetch = [&](int jj) -> int {
        const bool exists = jj >= 0 && jj < npad;
        if constexpr ((64 * B * G + HADI_ROW_PAD(B, (int)sizeof(T))) % (16 / (int)sizeof(T)) == 0)
            hadi_row_to_lds_fixed<B, T, G>(Ub + (ptrdiff_t)jj * rowp, slot(jj), lane, exists);
        else
            hadi_row_to_lds(Ub + (size_t)jj * rowp, slot(jj), rowp, lane, exists);
        return exists ? hadi_row_dma_count<T>(rowp) : 0;
    };
    // prologue: rows of iterations 0 .. PD-1
    if (iters > 0)
        for (int rr = wv; rr < PD * W + 4; rr += W * G) fetch(j0 - 2 + rr);

    // Vector-memory operations retire in issue order.  ya[k] = (lower bound of the) number of operations this
    // wavefront issued after the DMA batch that iteration it+k needs, so hadi_wait_vmcnt(ya[0]) retires that
    // batch and leaves younger batches and result stores in flight.
    int ya[PD];
#pragma unroll
    for (int k = 0; k < PD; k++) ya[k] = 0;
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    unsigned long long stamp_store_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    c.stamp_acc_ = stamp_store_;
#endif
    HADI_STAMP_DECL(stamp_store_)
    HADI_STAMP(8);  // prologue
    for (int it = 0; it < iters_all; it++) {
        const int J = j0 + it * W;
        hadi_wait_vmcnt(ya[0]);
        __syncthreads();  // this iteration's rows have landed; everyone is done with the rows replaced below
        HADI_STAMP(9);  // barrier wait (incl. DMA drain)
        int z = 0;
        if (it + PD < iters && wv < W) z = fetch(J + PD * W + 2 + wv);
#pragma unroll
        for (int k = 0; k + 1 < PD; k++) ya[k] = ya[k + 1] + z;
        ya[PD - 1] = 0;
        if constexpr (PD == 1) ya[0] = 0;
        const int j = J + wrow;
        const bool active = it < iters && j < j1;
        if constexpr (G == 1) {
            if (!active) continue;
        }
        if (j == nrows - 1)
            hadi_row_step<B, G, AMER, true, MODE, T, SCH>(c, active, j, slot(j - 2), slot(j - 1), slot(j), slot(j + 1), slot(j + 2));
        else
            hadi_row_step<B, G, AMER, false, MODE, T, SCH>(c, active, j, slot(j - 2), slot(j - 1), slot(j), slot(j + 1), slot(j + 2));
        if (active) {  // B/2 (one for B = 1) vector stores of the block; the i = 0 store is not counted (lower bound)
#pragma unroll
            for (int k = 0; k < PD; k++) ya[k] += hadi_put_block_stores<B, T>();
        }
        HADI_STAMP(10);  // whole row step (+ fetch issue)
    }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    if (lane == 0)
        for (int k = 0; k < 12; k++) atomicAdd(&g_hadi_stamps[k], stamp_store_[k]);
#endif
