// hadi_k_lds_seq.h -- what the one-wavefront LDS kernels of the small grids share (hadi_small_seq_kernel, hadi_small_seq2_kernel,
// hadi_small_sch_kernel): the back substitution of the row sweep and the pentadiagonal column sweep of all three; stage-in /
// stage-out of an instance in the natural-order layout and the lane's row-table entry of the two Douglas kernels.  (The forward
// row sweep of the two Douglas kernels is hadi_k_lds_row_body.h, included into both; hadi_small_sch_kernel's `rows` has its own
// node formulas, and that kernel keeps stage-in / stage-out and the table load written out, which the helpers made measurably
// slower: DESIGN.md section 5, "Small-grid kernels on shared pieces".)
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// ---- stage-in / stage-out: one instance between its packed global arrays and the natural-order layout at `base` -----------
// LY: HadiSmallSeqLayout (pitch, off_coef, off_b2, off_ptab; the state field starts at 0).  The caller has
// zeroed the whole layout and put a barrier behind that; all 64 lanes copy.
template <int B, class LY>
HADI_DEV HADI_FORCEINLINE void hadi_lds_stage_in(double *base, const LY &Ls, const HadiSweepArgs &a, int inst, int lane) {
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1, PL = Ls.pitch;
    const double *__restrict__ Ug = a.U + (size_t)inst * a.L.inst_stride;
    for (int e = lane; e < nrows * (m1 + 1); e += 64) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        base[j * PL + i] = Ug[(size_t)j * rowp + hadi_pos(B, 1, i)];
    }
    const double *__restrict__ sc = a.scoef + (size_t)inst * 4 * 64 * B;
    for (int e = lane; e < 4 * (m1 + 1); e += 64) {  // [i][4]: Bm, Bp, Dm, Dp of node i
        const int i = e >> 2, k = e & 3;
        base[Ls.off_coef + e] = (i >= 1) ? sc[k * 64 * B + hadi_pos(B, 1, i)] : 0.0;
    }
    const double *__restrict__ b2g = a.b2row + (size_t)inst * rowp;
    for (int i = lane; i <= m1; i += 64) base[Ls.off_b2 + i] = b2g[hadi_pos(B, 1, i)];
    const double *__restrict__ pg = a.pb + (size_t)inst * a.L.nrows_pad * HADI_PBW;
    for (int e = lane; e < nrows * 5; e += 64) base[Ls.off_ptab + e] = pg[(e / 5) * HADI_PBW + e % 5];  // [k][5]: L, L2, Q, C, C2
}
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_lds_stage_out(const double *base, int PL, const HadiSweepArgs &a, int inst, int lane) {
    const int nrows = a.L.nrows, rowp = a.L.rowp, m1 = a.L.m1;
    double *__restrict__ Ug = a.U + (size_t)inst * a.L.inst_stride;
    for (int e = lane; e < nrows * (m1 + 1); e += 64) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        Ug[(size_t)j * rowp + hadi_pos(B, 1, i)] = base[j * PL + i];
    }
}

// ---- this lane's v-row: its table entry stays in registers for the whole time loop (all zero for a lane without a row) -----
struct HadiLdsRowTab {
    double v, wm, wz, wp, a2l2, a2l1, a2m, a2u1, a2u2, b1val;
    int b1col;     // the interior column that carries b1 on this v-row, -1 if none
    bool b1_at0;   // ... and whether column 0 does
};
HADI_DEV HADI_FORCEINLINE HadiLdsRowTab hadi_lds_row_table(const HadiSweepArgs &a, int inst, int j, bool act) {
    HadiLdsRowTab t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1, false};
    if (act) {
        const double *__restrict__ rc = a.rowc + ((size_t)inst * a.L.nrows + j) * HADI_RC;
        t.v = rc[RC_V]; t.wm = rc[RC_WM]; t.wz = rc[RC_WZ]; t.wp = rc[RC_WP];
        t.a2l2 = rc[RC_L2]; t.a2l1 = rc[RC_L1]; t.a2m = rc[RC_M]; t.a2u1 = rc[RC_U1]; t.a2u2 = rc[RC_U2];
        t.b1val = rc[RC_B1VAL];
        const int b1raw = (int)rc[RC_B1COL];
        t.b1_at0 = b1raw == 0 || b1raw >= HADI_B1_BOTH;  // (two entries on one v-row: m2 > m1 only)
        t.b1col = b1raw >= HADI_B1_BOTH ? b1raw - HADI_B1_BOTH : b1raw;
    }
    return t;
}

// ---- the end of a row sweep: back substitution on the output itself, Y_i = g_i - c'_i Y_{i+1}, then column 0 (the forward
// sweep left g_i in yrow and c'_i in column i - 1 of crow; lanes without a row walk their dummy row) -------------------------
HADI_DEV HADI_FORCEINLINE void hadi_lds_back_subst(double *yrow, const double *crow, int m1, double yout_c0) {
    double Yn = yrow[m1];
    int i = m1 - 1;
    for (; i >= 8; i -= 8) {  // eight nodes per round: 16 independent LDS reads, then the dependent FMAs
        double g[8], cq[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { g[q] = yrow[i - q]; cq[q] = crow[i - q - 1]; }
#if !defined(HADI_EMU)
        asm volatile("" ::: "memory");
#endif
#pragma unroll
        for (int q = 0; q < 8; q++) {
            Yn = fma(-cq[q], Yn, g[q]);
            yrow[i - q] = Yn;
        }
    }
    for (; i >= 1; i--) {
        Yn = fma(-crow[i - 1], Yn, yrow[i]);
        yrow[i] = Yn;
    }
    yrow[0] = yout_c0;
}

// ---- the column sweep: lane <-> s-column, sequential pentadiagonal sweeps Y -> U (hes_a2_shuffled_kernels.hpp:243-299) ------
// ptab: [k][5] = L, L2, Q, C, C2 of v-row k; Y and U in natural order with pitch PL; all 64 lanes of the wavefront.
// (measured and left out, 50x25 x3000: fetching a node's coefficients one iteration ahead 2.64 -> 2.72 ms; the column
// held in 33 registers with all loads up front 2.64 -> 2.88 ms)
HADI_DEV HADI_FORCEINLINE void hadi_lds_penta_cols(double *Y, double *U, const double *ptab, int PL, int nrows, int m1, int lane) {
    for (int col = lane; col <= m1; col += 64) {
        // eight rows per round: the independent LDS reads first, then the dependent recurrence
        double ym1 = 0.0, ym2 = 0.0;
        int k = 0;
        for (; k + 8 <= nrows; k += 8) {
            double yv[8], tL[8], tL2[8], tQ[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {  // (the round's table entries with its column values: 32 reads, one wait)
                const double *t = ptab + (k + q) * 5;
                yv[q] = Y[(k + q) * PL + col];
                tL[q] = t[PB_L]; tL2[q] = t[PB_L2]; tQ[q] = t[PB_Q];
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");
#endif
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const double yk = (yv[q] - tL[q] * ym1 - tL2[q] * ym2) * tQ[q];
                Y[(k + q) * PL + col] = yk;
                ym2 = ym1;
                ym1 = yk;
            }
        }
        for (; k < nrows; k++) {
            const double *t = ptab + k * 5;
            const double yk = (Y[k * PL + col] - t[PB_L] * ym1 - t[PB_L2] * ym2) * t[PB_Q];
            Y[k * PL + col] = yk;
            ym2 = ym1;
            ym1 = yk;
        }
        double xp1 = 0.0, xp2 = 0.0;
        k = nrows - 1;
        for (; k >= 7; k -= 8) {
            double yv[8], tC[8], tC2[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const double *t = ptab + (k - q) * 5;
                yv[q] = Y[(k - q) * PL + col];
                tC[q] = t[PB_C]; tC2[q] = t[PB_C2];
            }
#if !defined(HADI_EMU)
            asm volatile("" ::: "memory");
#endif
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const double xk = yv[q] - tC[q] * xp1 - tC2[q] * xp2;
                xp2 = xp1;
                xp1 = xk;
                U[(k - q) * PL + col] = xk;
            }
        }
        for (; k >= 0; k--) {
            const double *t = ptab + k * 5;
            const double xk = Y[k * PL + col] - t[PB_C] * xp1 - t[PB_C2] * xp2;
            xp2 = xp1;
            xp1 = xk;
            U[k * PL + col] = xk;
        }
    }
}
