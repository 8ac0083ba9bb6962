// hadi_k_small_sch.h -- LDS-resident kernel of the predictor-corrector schemes on the calibration-size grids (hadi_small_sch_kernel).
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// ------------------------------------------------------------------------------------------------
// Small grids, Craig-Sneyd / Modified Craig-Sneyd / Hundsdorfer-Verwer sweeps (European call data, fp64): ONE wavefront per
// instance and ONE launch for the whole time loop, built like hadi_small_seq_kernel -- row sweeps lane <-> v-row (sliding
// window, v-neighbours by wave shifts, Thomas in the lane), column sweeps lane <-> s-column with the factors of `pb`.  A step
// is two such row / column pairs.  With e_n = exp(bc_rate dt n), b0 = 0 and beta = 0 (CS), 1/2 - theta (MCS), 1/2 (HV):
//   predictor  the Douglas step on U: Y0, the A1 solve, + C2, the A2 solve -> V = Y2, where
//                C2 = theta dt (b2 (e_n - e_{n-1}) - A2 U)
//              and, folded by the same row sweep from the operators it has at hand, everything the corrector needs of U:
//                CS, MCS  R1 = U + dt/2 A0U + (1 - beta - theta) dt A1U + (1 - beta) dt A2U
//                              + b2 (dt e_{n-1} + beta dt (e_n - e_{n-1})) + b1 (the same + theta dt (e_n - e_{n-1}))
//                HV       R1 = U + dt/2 (A0U + A1U + A2U) + b dt/2 (e_{n-1} + e_n)
//   corrector  row sweep on V: right-hand side R1 + dt/2 A0V + g1 A1V + g2 A2V (CS g1 = g2 = 0; MCS g1 = g2 = beta dt; HV
//              g1 = (1/2 - theta) dt, g2 = dt/2), the A1 solve, + C2 (HV: - theta dt A2V), the A2 solve -> the new U.
// (tests/scheme_ref.py states the step; the fold is its Y-hat and the two implicit stages' right-hand sides written out.)
// LDS, natural order, odd pitch: four fields -- UV (U, then V, then the new U), Y (the sweeps' work array), R1, C2 -- and the
// staged tables.  The forward sweep parks c'_i in column i - 1 of the UV row it walks and g_i in Y, exactly as
// hadi_small_seq_kernel does; both column sweeps rebuild UV completely.  R1 and C2 are written and read by the lane that owns
// the v-row: no other lane touches them.
struct HadiSmallSchLayout {
    int pitch;  // doubles per row: odd, >= m1 + 3 (columns m1 + 1, m1 + 2 stay zero in every field)
    int off_y, off_r1, off_c2, off_coef, off_b2, off_zero, off_dummy, off_ptab, total;  // offsets in doubles: UV starts at 0
};
HADI_HD inline HadiSmallSchLayout hadi_small_sch_layout(int m1, int nrows) {
    HadiSmallSchLayout l;
    l.pitch = (m1 + 3) | 1;
    const int field = nrows * l.pitch;
    l.off_y = field;
    l.off_r1 = 2 * field;
    l.off_c2 = 3 * field;
    l.off_coef = (4 * field + 1) & ~1;  // 16-byte aligned quads
    l.off_b2 = l.off_coef + 4 * (m1 + 2);
    l.off_zero = l.off_b2 + (m1 + 2);     // a row of zeros: the "b2 row" of every v-row but the last
    l.off_dummy = l.off_zero + (m1 + 2);  // where the idle lanes (>= nrows) put their results (emulator only)
    l.off_ptab = l.off_dummy + l.pitch;
    l.total = l.off_ptab + nrows * 5;
    return l;
}

template <int V>
struct HadiSchStage { static constexpr int value = V; };  // 1 predictor, 2 corrector

template <int B, int SCH>
__global__ void __launch_bounds__(64) hadi_small_sch_kernel(HadiSweepArgs a, HadiSmallArgs sm) {
    static_assert(SCH == HADI_SCH_CS || SCH == HADI_SCH_MCS || SCH == HADI_SCH_HV, "CS, MCS or HV");
    HADI_DYN_SMEM(double, smem);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.n_inst) return;
    const int inst = sm.order ? sm.order[blockIdx.x] : (int)blockIdx.x;
    const HadiInstPar ip = a.ipar[inst];
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1;
    const HadiSmallSchLayout Ls = hadi_small_sch_layout(m1, nrows);
    const int PL = Ls.pitch;
    double *Ul = smem;  // row 0 of UV
    double *Yl = smem + Ls.off_y;
    double *coefl = smem + Ls.off_coef;  // [i][4]: Bm, Bp, Dm, Dp of node i
    double *b2l = smem + Ls.off_b2;
    double *ptab = smem + Ls.off_ptab;   // [k][5]: L, L2, Q, C, C2
    double *__restrict__ Ug = a.U + (size_t)inst * a.L.inst_stride;

    for (int e = lane; e < Ls.total; e += 64) smem[e] = 0.0;
    __syncthreads();
    // Stage-in, the row-table load and the stage-out below are hadi_lds_stage_in / hadi_lds_row_table / hadi_lds_stage_out
    // (hadi_k_lds_seq.h) written out: through the helpers this kernel's register allocation changed (<1,CS> 171 -> 245 VGPRs,
    // one more wait in the MCS time loop) and MCS measured 0.6 % slower; written out the stream is the earlier one
    // ("Small-grid kernels on shared pieces").
    for (int e = lane; e < nrows * (m1 + 1); e += 64) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        Ul[j * PL + i] = Ug[(size_t)j * rowp + hadi_pos(B, 1, i)];
    }
    {
        const double *__restrict__ sc = a.scoef + (size_t)inst * 4 * 64 * B;
        for (int e = lane; e < 4 * (m1 + 1); e += 64) {
            const int i = e >> 2, k = e & 3;
            coefl[e] = (i >= 1) ? sc[k * 64 * B + hadi_pos(B, 1, i)] : 0.0;
        }
        const double *__restrict__ b2g = a.b2row + (size_t)inst * rowp;
        for (int i = lane; i <= m1; i += 64) b2l[i] = b2g[hadi_pos(B, 1, i)];
        const double *__restrict__ pg = a.pb + (size_t)inst * a.L.nrows_pad * HADI_PBW;
        for (int e = lane; e < nrows * 5; e += 64) ptab[e] = pg[(e / 5) * HADI_PBW + e % 5];
    }
    // this lane's v-row: its table entry stays in registers for the whole time loop
    const int j = lane;
    const bool act = j < nrows;
    const bool last = (j == nrows - 1);
    double v = 0.0, wm = 0.0, wz = 0.0, wp = 0.0, a2l2 = 0.0, a2l1 = 0.0, a2m = 0.0, a2u1 = 0.0, a2u2 = 0.0, b1val = 0.0;
    int b1col = -1;
    bool b1_at0 = false;
    if (act) {
        const double *__restrict__ rc = a.rowc + ((size_t)inst * nrows + j) * HADI_RC;
        v = rc[RC_V]; wm = rc[RC_WM]; wz = rc[RC_WZ]; wp = rc[RC_WP];
        a2l2 = rc[RC_L2]; a2l1 = rc[RC_L1]; a2m = rc[RC_M]; a2u1 = rc[RC_U1]; a2u2 = rc[RC_U2];
        b1val = rc[RC_B1VAL];
        const int b1raw = (int)rc[RC_B1COL];
        b1_at0 = b1raw == 0 || b1raw >= HADI_B1_BOTH;  // (two entries on one v-row: m2 > m1 only)
        b1col = b1raw >= HADI_B1_BOTH ? b1raw - HADI_B1_BOTH : b1raw;
    }
    const double dt = ip.dt, thdt = ip.thdt, qd = ip.q, half_rd = ip.half_rd;
    // the scheme's constants (wave-uniform): see the head of this file
    const double hdt = 0.5 * dt;
    const double bdt = SCH == HADI_SCH_CS ? 0.0 : SCH == HADI_SCH_MCS ? hdt - thdt : hdt;
    const double k1 = SCH == HADI_SCH_HV ? hdt : dt - bdt - thdt;
    const double k2 = SCH == HADI_SCH_HV ? hdt : dt - bdt;
    const double g1 = SCH == HADI_SCH_HV ? hdt - thdt : bdt;
    const double g2 = bdt;
    const double *urow = Ul + (act ? j : 0) * PL;  // (idle lanes walk row 0 and store nothing that counts)
    // The v-neighbours j-2 .. j+2 of a column are the same column in the neighbouring lanes' rows (hadi_small_seq_kernel): beyond
    // the grid the shifts deliver 0 or an idle lane's (finite) value of row 0, which only ever meets a zero weight.
    auto col5 = [&](const double own, double &m2v, double &m1v, double &p1v, double &p2v) {
        m1v = hadi_lane_prev(own); m2v = hadi_lane_prev(m1v);
        p1v = hadi_lane_next(own); p2v = hadi_lane_next(p1v);
    };
    double *dummy = smem + Ls.off_dummy;
    double *yrow = act ? Yl + j * PL : dummy;                  // (idle lanes store into a dummy row)
    double *crow = act ? Ul + j * PL : dummy;                  // column i - 1 of this row receives c'_i
    double *r1row = act ? smem + Ls.off_r1 + j * PL : dummy;   // the carry-over rows of this v-row
    double *c2row = act ? smem + Ls.off_c2 + j * PL : dummy;
    const double *b2p = last ? b2l : smem + Ls.off_zero;       // b2 lives on the last v-row only
    __syncthreads();

    // ---- one row sweep: lane <-> v-row, i = 1 .. m1; `stage` 1 walks U (predictor), 2 walks V (corrector) -----------------
    auto rows = [&](auto stage, const double e_nm1, const double e_n) {
        constexpr bool PRED = decltype(stage)::value == 1;
        constexpr bool HV = SCH == HADI_SCH_HV;
        const double de = e_n - e_nm1;
        const double b1l = b1val * (dt * e_nm1 + thdt * de);  // predictor's right-hand side: b1 dt e_{n-1} + theta dt b1 (e_n - e_{n-1})
        const double cb2r = fma(bdt, de, dt * e_nm1);         // R1's boundary weights
        const double cb1r = HV ? cb2r : cb2r + thdt * de;
        const double b1r = b1val * cb1r;
        // column i = 0 (A0 and A1 rows are zero there: only A2 and the boundary act, and the A1 solve is the identity)
        const double c00 = urow[0];
        double c0m2, c0m1, c0p1, c0p2;
        col5(c00, c0m2, c0m1, c0p1, c0p2);
        double r_0 = urow[1], r_m2, r_m1, r_p1, r_p2;
        col5(r_0, r_m2, r_m1, r_p1, r_p2);
        double yout_c0, x0;
        {
            const double a2c0 = a2l2 * c0m2 + a2l1 * c0m1 + a2m * c00 + a2u1 * c0p1 + a2u2 * c0p2;
            double c2c0;
            if constexpr (PRED) {
                const double b1c0 = b1_at0 ? b1val : 0.0;
                const double b2c0 = b2p[0];
                x0 = c00 + dt * (a2c0 + (b1c0 + b2c0) * e_nm1) + thdt * (b1c0 * de);
                c2c0 = thdt * (b2c0 * e_n - (a2c0 + b2c0 * e_nm1));
                r1row[0] = c00 + k2 * a2c0 + cb2r * b2c0 + cb1r * b1c0;
                c2row[0] = c2c0;
            } else {
                x0 = fma(g2, a2c0, r1row[0]);
                c2c0 = HV ? -thdt * a2c0 : c2row[0];
            }
            yout_c0 = x0 + c2c0;
        }
        hadi_wave_rendezvous();  // (emulator: everyone has read column 0 and 1 before c' overwrites column 0)
        double u_prev = c00, u_cur = r_0;
        double t_prev = wm * c0m1 + wz * c00 + wp * c0p1;
        double t_cur = wm * r_m1 + wz * r_0 + wp * r_p1;
        double a2u_cur = fma(a2u2, r_p2, fma(a2l2, r_m2, a2l1 * r_m1 + a2m * r_0 + a2u1 * r_p1));
        double b2c = PRED ? b2p[1] : 0.0;
        double corr_cur;
        if constexpr (PRED) corr_cur = thdt * (b2c * e_n - (a2u_cur + b2c * e_nm1));
        else corr_cur = HV ? -thdt * a2u_cur : c2row[1];
        // raw values of column 2 (column m1 + 1 is the zero spare)
        r_0 = urow[2];
        col5(r_0, r_m2, r_m1, r_p1, r_p2);
        double cp_prev = 0.0, ys_prev = x0;  // (x_0 is known: with ys_0 = x_0 and c'_0 = 0 the general step moves it to the right-hand side)
        // One node.  On entry r_* hold the raw column i + 1; cB, cD are node i's coefficients; predictor: b2n the b2 entry of node
        // i + 1; corrector: r1v = R1 of node i, c2n = C2 of node i + 1.  The caller refills r_* with column i + 2 afterwards.
        auto node = [&](int i, const double2 cB, const double2 cD, const double b2n, const double r1v, const double c2n) {
            const double u_next = r_0;
            const double t_next = wm * r_m1 + wz * r_0 + wp * r_p1;
            const double a2u_next = fma(a2u2, r_p2, fma(a2l2, r_m2, a2l1 * r_m1 + a2m * r_0 + a2u1 * r_p1));
            const double lo = fma(v, cD.x, qd * cB.x);
            const double up = fma(v, cD.y, qd * cB.y);
            const double mn = -((lo + up) + half_rd);
            const double A1U = lo * u_prev + mn * u_cur + up * u_next;
            const double A0U = cB.x * t_prev - (cB.x + cB.y) * t_cur + cB.y * t_next;
            double y, corr_next;
            if constexpr (PRED) {
                // Y0 + theta dt (b1 e_n - (A1U + b1 e_{n-1})), as hadi_small_seq_kernel forms it
                double S = A0U + A1U + a2u_cur;
                S += b2c * e_nm1;
                y = fma(dt, S, u_cur);
                y = fma(-thdt, A1U, y);
                y += (i == b1col) ? b1l : 0.0;
                double r1 = fma(hdt, A0U, u_cur);
                r1 = fma(k1, A1U, r1);
                r1 = fma(k2, a2u_cur, r1);
                r1 = fma(cb2r, b2c, r1);
                r1 += (i == b1col) ? b1r : 0.0;
                r1row[i] = r1;
                c2row[i] = corr_cur;
                corr_next = thdt * (b2n * e_n - (a2u_next + b2n * e_nm1));
            } else {
                y = fma(hdt, A0U, r1v);
                if constexpr (SCH != HADI_SCH_CS) y = fma(g2, a2u_cur, fma(g1, A1U, y));
                corr_next = HV ? -thdt * a2u_next : c2n;
            }
            const double il = -thdt * lo;
            const double im = 1.0 - thdt * mn;
            const double iu = -thdt * up;
            const double inv = hadi_rcp(fma(-il, cp_prev, im));
            const double cp = iu * inv;
            const double ys = fma(-il, ys_prev, y) * inv;
            yrow[i] = ys + corr_cur + cp * corr_next;  // g_i  (c'_{m1} = 0: the row ends there)
            crow[i - 1] = cp;
            u_prev = u_cur; u_cur = u_next;
            t_prev = t_cur; t_cur = t_next;
            a2u_cur = a2u_next; corr_cur = corr_next; b2c = b2n;
            cp_prev = cp; ys_prev = ys;
        };
        // Rounds of four nodes: all LDS reads of the round first, behind one wait, then the four dependent steps.  Column indices
        // reach i + 5 <= m1 + 2: the two zero spare columns of the pitch (C2's column m1 + 1 is never written: zero).
        int i = 1;
        for (; i + 3 <= m1; i += 4) {
            double Rm2[4], Rm1[4], R0[4], Rp1[4], Rp2[4], b2q[4], r1q[4], c2q[4];
            double2 cBq[4], cDq[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                R0[q] = urow[i + 2 + q];
                cBq[q] = *reinterpret_cast<const double2 *>(coefl + 4 * (i + q));
                cDq[q] = *reinterpret_cast<const double2 *>(coefl + 4 * (i + q) + 2);
                b2q[q] = PRED ? b2p[i + 1 + q] : 0.0;  // (entry m1 + 1 is zero)
                r1q[q] = PRED ? 0.0 : r1row[i + q];
                c2q[q] = (PRED || HV) ? 0.0 : c2row[i + 1 + q];
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");  // (the reads stay in front of the four steps' stores)
#endif
            hadi_wave_rendezvous();  // (emulator: every lane has read its columns before anybody's c' lands in them)
#pragma unroll
            for (int q = 0; q < 4; q++) col5(R0[q], Rm2[q], Rm1[q], Rp1[q], Rp2[q]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                node(i + q, cBq[q], cDq[q], b2q[q], r1q[q], c2q[q]);
                r_m2 = Rm2[q]; r_m1 = Rm1[q]; r_0 = R0[q]; r_p1 = Rp1[q]; r_p2 = Rp2[q];
                hadi_wave_rendezvous();  // (emulator: the lanes walk in lock step on the GPU)
            }
        }
        for (; i <= m1; i++) {  // the last m1 mod 4 nodes, one at a time
            const double n_0 = urow[i + 2];  // (column <= m1 + 2: a zero column)
            double n_m2, n_m1, n_p1, n_p2;
            col5(n_0, n_m2, n_m1, n_p1, n_p2);
            const double2 cB = *reinterpret_cast<const double2 *>(coefl + 4 * i);      // Bm, Bp
            const double2 cD = *reinterpret_cast<const double2 *>(coefl + 4 * i + 2);  // Dm, Dp
            const double b2n = PRED ? b2p[i + 1] : 0.0;
            const double r1v = PRED ? 0.0 : r1row[i];
            const double c2n = (PRED || HV) ? 0.0 : c2row[i + 1];
            hadi_wave_rendezvous();
            node(i, cB, cD, b2n, r1v, c2n);
            r_m2 = n_m2; r_m1 = n_m1; r_0 = n_0; r_p1 = n_p1; r_p2 = n_p2;
            hadi_wave_rendezvous();  // (emulator: the lanes walk in lock step on the GPU)
        }
        hadi_lds_back_subst(yrow, crow, m1, yout_c0);
    };
    // ---- one column sweep: lane <-> s-column, Y -> UV ----
    auto cols = [&]() { hadi_lds_penta_cols(Yl, Ul, ptab, PL, nrows, m1, lane); };

    // Only the lanes that own a v-row run the row sweeps (the wave shifts deliver 0 from a switched-off lane).  The emulator's
    // lane threads all have to take part in its collective shuffles, so there every lane runs.
#if defined(HADI_EMU)
    const bool rowrun = true;
#else
    const bool rowrun = act;
#endif
    const int N = ip.N < sm.Nmax ? ip.N : sm.Nmax;
    HadiSnapCursor snap = hadi_snap_begin(sm);
    const int snap_off = sm.n_snap > 0 ? hadi_snap_natural(a.L, sm.snap_node[inst], PL) : -1;
    for (int n = 1; n <= N; n++) {
        const double e_nm1 = exp(ip.bc_rate * ip.dt * (n - 1));
        const double e_n = exp(ip.bc_rate * ip.dt * n);
        if (rowrun) rows(HadiSchStage<1>{}, e_nm1, e_n);  // predictor: U -> Y (and R1, C2)
        __syncthreads();
        cols();                                           // Y -> V = Y2
        __syncthreads();
        if (rowrun) rows(HadiSchStage<2>{}, e_nm1, e_n);  // corrector: V, R1, C2 -> Y
        __syncthreads();
        cols();                                           // Y -> the new U
        __syncthreads();
        if (hadi_ex_listed(sm.ex_flag, sm.ex_stride, inst, n)) {  // Bermudan exercise behind the corrector's column pass (wave-uniform)
            hadi_exercise_lds<B>(Ul, PL, true, a.U0 + (size_t)inst * a.L.inst_stride, nrows, m1, rowp, lane, 64);
            __syncthreads();
        }
        if (hadi_ex_listed(sm.ko_flag, sm.ko_stride, inst, n)) {  // knock-out behind the corrector's column pass (wave-uniform)
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
    for (int e = lane; e < nrows * (m1 + 1); e += 64) {
        const int jj = e / (m1 + 1), i = e - jj * (m1 + 1);
        Ug[(size_t)jj * rowp + hadi_pos(B, 1, i)] = Ul[jj * PL + i];
    }
}
