// hadi_k_greeks.h -- Greeks and the spot ladder of row V_0, once after the sweep (hadi_compute_greeks, include/hadi.h).
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// Columns of one ladder row (enum hadi_greek of hadi.h).
enum { HADI_GK_PRICE = 0, HADI_GK_DELTA = 1, HADI_GK_GAMMA = 2, HADI_GK_DV = 3, HADI_GK_DVV = 4, HADI_GK_DSV = 5,
       HADI_GK_THETA = 6, HADI_GK_LAMBDA = 7, HADI_GK_N = 8 };
#define HADI_GK_THREADS 256
#define HADI_GK_TILE 512  // s-nodes per block on the rows kept in natural order (hadi_pick_shape: B = 1); permuted rows are one tile
#define HADI_GK_HALO 2    // the one-sided s-stencils of the end nodes reach two nodes inwards

struct HadiGreeksArgs {
    HadiLayout L;
    int n_inst, ntiles, span;  // span = doubles per staged row: L.rowp (permuted rows), HADI_GK_TILE + 2 HADI_GK_HALO (natural rows)
    int american;
    const double *U, *LAM;                       // packed state after the last step (LAM: American sweeps only)
    const double *scoef, *b2row, *rowc;          // the sweep's operator tables (hadi_setup_instance)
    const HadiInstPar *ipar;
    const double *vec_s, *vec_v, *delta_s, *delta_v;
    double S_0, V_0;
    double *greeks;  // [n][8]
    double *ladder;  // [n][m1+1][8] or nullptr
    int *status;     // [n]: 0 ok, 1 S_0 is not an s-node, 2 V_0 is not a v-node
};
HADI_HD inline size_t hadi_greeks_smem(int span) { return ((size_t)6 * span + HADI_GK_THREADS) * sizeof(double); }

// Three-point weights of the first (w1) and second (w2) derivative at node k of an axis with m intervals D[0 .. m-1]; they act
// on the nodes base, base + 1, base + 2.  Interior: beta / delta of coeff.hpp; k = 0: gamma; k = m: alpha; the second
// derivative of an end node is its interior neighbour's (one parabola through the three nodes).
HADI_HD inline int hadi_greek_weights(const double *D, int m, int k, double *w1, double *w2) {
    const int kc = k < 1 ? 1 : (k > m - 1 ? m - 1 : k);  // centre of the three nodes
    w2[0] = hadi_fd_delta(D, kc - 1, -1); w2[1] = hadi_fd_delta(D, kc - 1, 0); w2[2] = hadi_fd_delta(D, kc - 1, 1);
    if (k == 0) {
        w1[0] = hadi_fd_gamma(D, -1, 0); w1[1] = hadi_fd_gamma(D, -1, 1); w1[2] = hadi_fd_gamma(D, -1, 2);
    } else if (k == m) {
        w1[0] = hadi_fd_alpha(D, m - 1, -2); w1[1] = hadi_fd_alpha(D, m - 1, -1); w1[2] = hadi_fd_alpha(D, m - 1, 0);
    } else {
        w1[0] = hadi_fd_beta(D, k - 1, -1); w1[1] = hadi_fd_beta(D, k - 1, 0); w1[2] = hadi_fd_beta(D, k - 1, 1);
    }
    return kc - 1;
}

// One block per (instance, s-tile).  The rows j0 - 2 .. j0 + 2 of U (clipped to the grid; j0 = the v-node of V_0) and the row
// j0 of lambda_bar -- the only one its two columns read -- are staged into LDS in storage order, so the loads coalesce; the
// s-neighbours of a node, which the packed layout scatters over the row, then come from LDS through hadi_pos.  Rows of at most
// 1024 intervals are staged whole (one tile); the rows of the sequential shapes are in natural order and are cut into tiles
// of HADI_GK_TILE nodes with a halo.  Delta, gamma and the v-derivatives take their weights from the grid arrays; theta is
// minus the explicit right-hand side of the sweep, evaluated per node from the sweep's own tables exactly as the explicit
// stage of hadi_pass_a_seq states it.  Without a ladder only the thread that owns the node of S_0 evaluates anything.
__global__ void __launch_bounds__(HADI_GK_THREADS) hadi_greeks_kernel(HadiGreeksArgs g) {
    HADI_DYN_SMEM(double, sm);
    const HadiLayout &L = g.L;
    const int tid = threadIdx.x, nth = blockDim.x;
    if ((int)blockIdx.x >= g.n_inst * g.ntiles) return;
    const int inst = blockIdx.x / g.ntiles, tile = blockIdx.x - inst * g.ntiles;
    const int m1 = L.m1, m2 = L.m2, rowp = L.rowp, nslot = 64 * L.B * L.G, span = g.span;
    const bool natural = L.B == 1;
    double *rows = sm;                    // [5][span]
    double *lamrow = sm + (size_t)5 * span;  // [span]
    int *red = reinterpret_cast<int *>(sm + (size_t)6 * span);  // [2][HADI_GK_THREADS]
    const double *vs = g.vec_s + (size_t)inst * (m1 + 1), *vv = g.vec_v + (size_t)inst * (m2 + 1);
    const double *ds = g.delta_s + (size_t)inst * m1, *dv = g.delta_v + (size_t)inst * m2;

    // the node of (S_0, V_0): first node within 1e-10, as hadi_pick_kernel looks it up
    {
        int fi = INT32_MAX, fj = INT32_MAX;
        for (int i = tid; i <= m1; i += nth)
            if (fabs(vs[i] - g.S_0) < 1e-10) { fi = i; break; }
        for (int j = tid; j <= m2; j += nth)
            if (fabs(vv[j] - g.V_0) < 1e-10) { fj = j; break; }
        red[tid] = fi;
        red[HADI_GK_THREADS + tid] = fj;
    }
    __syncthreads();
    int i0 = INT32_MAX, j0 = INT32_MAX;
    for (int k = 0; k < nth; k++) {
        i0 = red[k] < i0 ? red[k] : i0;
        j0 = red[HADI_GK_THREADS + k] < j0 ? red[HADI_GK_THREADS + k] : j0;
    }
    const bool off_s = i0 > m1, off_v = j0 > m2;
    if (off_s || off_v) {  // (block-uniform)
        if (tile == 0) {
            if (tid == 0) g.status[inst] = off_s ? 1 : 2;
            if (tid < HADI_GK_N) g.greeks[(size_t)inst * HADI_GK_N + tid] = nan("");
        }
        return;
    }
    if (tile == 0 && tid == 0) g.status[inst] = 0;
    // nodes of this tile, and the nodes its stencils read
    const int i_lo = natural ? tile * HADI_GK_TILE : 0;
    const int i_hi = natural ? (i_lo + HADI_GK_TILE - 1 < m1 ? i_lo + HADI_GK_TILE - 1 : m1) : m1;
    if (!g.ladder && (i0 < i_lo || i0 > i_hi)) return;  // (block-uniform)
    const int i_base = i_lo - HADI_GK_HALO > 0 ? i_lo - HADI_GK_HALO : 0;
    const int i_top = i_hi + HADI_GK_HALO < m1 ? i_hi + HADI_GK_HALO : m1;
    const int j_lo = j0 - 2 > 0 ? j0 - 2 : 0, j_hi = j0 + 2 < m2 ? j0 + 2 : m2;
    const double *Ub = g.U + (size_t)inst * L.inst_stride;
    const double *Lb = g.american ? g.LAM + (size_t)inst * L.inst_stride + (size_t)j0 * rowp : nullptr;
    // staging.  Permuted rows: LDS index = storage slot.  Natural rows: LDS index = i - i_base, storage slot i - 1 (i = 0: nslot)
    const int nload = natural ? i_top - i_base + 1 : nslot + 1;
    for (int k = tid; k < nload; k += nth) {
        const int slot = natural ? hadi_pos(L, i_base + k) : k;
        for (int r = 0; r <= j_hi - j_lo; r++) rows[(size_t)r * span + k] = Ub[(size_t)(j_lo + r) * rowp + slot];
        lamrow[k] = g.american ? Lb[slot] : 0.0;
    }
    __syncthreads();

    const HadiInstPar ip = g.ipar[inst];
    const double *sc = g.scoef + (size_t)inst * 4 * nslot;
    const double *b2g = g.b2row + (size_t)inst * rowp;
    const double *rc = g.rowc + ((size_t)inst * L.nrows + j0) * HADI_RC;
    // v-stencils of row j0 (the same for every node of the ladder)
    double wv1[3], wv2[3];
    const int jb = hadi_greek_weights(dv, m2, j0, wv1, wv2);
    const double *rv0 = rows + (size_t)(jb - j_lo) * span, *rv1 = rv0 + span, *rv2 = rv1 + span;  // rows jb, jb + 1, jb + 2
    // rows j0 - 2 .. j0 + 2 for the operators, clamped to the grid: a clamped row only ever meets a zero weight (hadi_pass_a_seq)
    const double *pm2 = rows + (size_t)((j0 - 2 > 0 ? j0 - 2 : 0) - j_lo) * span, *pm1 = rows + (size_t)((j0 - 1 > 0 ? j0 - 1 : 0) - j_lo) * span;
    const double *pr0 = rows + (size_t)(j0 - j_lo) * span;
    const double *pp1 = rows + (size_t)((j0 + 1 < m2 ? j0 + 1 : m2) - j_lo) * span, *pp2 = rows + (size_t)((j0 + 2 < m2 ? j0 + 2 : m2) - j_lo) * span;
    const double v = rc[RC_V], wm = rc[RC_WM], wz = rc[RC_WZ], wp = rc[RC_WP];
    const double a2l2 = rc[RC_L2], a2l1 = rc[RC_L1], a2m = rc[RC_M], a2u1 = rc[RC_U1], a2u2 = rc[RC_U2], b1val = rc[RC_B1VAL];
    const int b1raw = (int)rc[RC_B1COL];
    const bool b1_at0 = b1raw == 0 || b1raw >= HADI_B1_BOTH;
    const int b1col = b1raw >= HADI_B1_BOTH ? b1raw - HADI_B1_BOTH : b1raw;
    const bool last = j0 == m2;
    const double e_N = exp(ip.bc_rate * ip.dt * ip.N);
    auto li = [&](int i) -> int { return natural ? i - i_base : hadi_pos(L, i); };

    for (int i = i_lo + tid; i <= i_hi; i += nth) {
        if (!g.ladder && i != i0) continue;
        double ws1[3], ws2[3];
        const int ib = hadi_greek_weights(ds, m1, i, ws1, ws2);
        const int x0 = li(ib), x1 = li(ib + 1), x2 = li(ib + 2), xi = li(i);
        double out[HADI_GK_N];
        // s-derivatives of the three v-rows jb .. jb + 2 and of row j0
        const double d0 = ws1[0] * rv0[x0] + ws1[1] * rv0[x1] + ws1[2] * rv0[x2];
        const double d1 = ws1[0] * rv1[x0] + ws1[1] * rv1[x1] + ws1[2] * rv1[x2];
        const double d2 = ws1[0] * rv2[x0] + ws1[1] * rv2[x1] + ws1[2] * rv2[x2];
        const double u = pr0[xi];
        out[HADI_GK_PRICE] = u;
        out[HADI_GK_DELTA] = ws1[0] * pr0[x0] + ws1[1] * pr0[x1] + ws1[2] * pr0[x2];
        out[HADI_GK_GAMMA] = ws2[0] * pr0[x0] + ws2[1] * pr0[x1] + ws2[2] * pr0[x2];
        out[HADI_GK_DV] = wv1[0] * rv0[xi] + wv1[1] * rv1[xi] + wv1[2] * rv2[xi];
        out[HADI_GK_DVV] = wv2[0] * rv0[xi] + wv2[1] * rv1[xi] + wv2[2] * rv2[xi];
        out[HADI_GK_DSV] = wv1[0] * d0 + wv1[1] * d1 + wv1[2] * d2;
        // theta = -F(t_N, U_N), F = A0 U + A1 U + A2 U + b e_N + lambda_bar  (device_solver.hpp:236-250)
        const double lam = lamrow[xi];
        const double A2U = fma(a2u2, pp2[xi], fma(a2l2, pm2[xi], a2l1 * pm1[xi] + a2m * u + a2u1 * pp1[xi]));
        const double b2c = last ? b2g[hadi_pos(L, i)] : 0.0;
        double F;
        if (i == 0) {  // the A0 and A1 rows are empty there (put: the reaction term): only A2 and the boundary act
            const double b1c = b1_at0 ? b1val : 0.0;
            F = A2U - ip.hr0 * u + (b1c + b2c) * e_N + lam;
        } else {
            const int xm = li(i - 1), xp = i < m1 ? li(i + 1) : xi;
            const double nxt = i < m1 ? 1.0 : 0.0;  // the s-neighbour behind the last node reads as zero
            const int ps = hadi_pos(L, i);
            const double Bm = sc[0 * nslot + ps], Bp = sc[1 * nslot + ps], Dm = sc[2 * nslot + ps], Dp = sc[3 * nslot + ps];
            const double lo = fma(v, Dm, ip.q * Bm);
            const double up = fma(v, Dp, ip.q * Bp);
            const double mn = -((lo + up) + ip.half_rd);
            const double A1U = lo * pr0[xm] + mn * u + up * (nxt * pr0[xp]);
            const double t_prev = wm * pm1[xm] + wz * pr0[xm] + wp * pp1[xm];
            const double t_cur = wm * pm1[xi] + wz * u + wp * pp1[xi];
            const double t_next = nxt * (wm * pm1[xp] + wz * pr0[xp] + wp * pp1[xp]);
            const double A0U = Bm * t_prev - (Bm + Bp) * t_cur + Bp * t_next;
            F = A0U + A1U + A2U + b2c * e_N + lam;
            F += (i == b1col) ? b1val * e_N : 0.0;
        }
        out[HADI_GK_THETA] = -F;
        out[HADI_GK_LAMBDA] = lam;
        if (g.ladder) {
            double2 *dst = reinterpret_cast<double2 *>(g.ladder + ((size_t)inst * (m1 + 1) + i) * HADI_GK_N);
#pragma unroll
            for (int c = 0; c < HADI_GK_N / 2; c++) { double2 w; w.x = out[2 * c]; w.y = out[2 * c + 1]; dst[c] = w; }
        }
        if (i == i0) {
            double2 *dst = reinterpret_cast<double2 *>(g.greeks + (size_t)inst * HADI_GK_N);
#pragma unroll
            for (int c = 0; c < HADI_GK_N / 2; c++) { double2 w; w.x = out[2 * c]; w.y = out[2 * c + 1]; dst[c] = w; }
        }
    }
}
