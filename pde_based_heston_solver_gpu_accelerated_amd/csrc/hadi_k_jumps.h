// hadi_k_jumps.h -- the Bates model: compound-Poisson lognormal jumps in the spot as a dense sub-step at the end of every step.
// In time to maturity the PIDE is u_t = L_Heston u + lambda (E[u(s Y)] - u - kbar s u_s), ln Y ~ N(mu, sigma^2),
// kbar = exp(mu + sigma^2 / 2) - 1.  One step of a jump call is the library's step, exactly as without jumps, and then, on every
// v-row of every instance that has not finished and whose a_k = lambda_k dt_k is not zero,
//     U_row <- U_row + a_k (G U_row),    G = J - I - kbar diag(s) D,  row 0 (s = 0) all zero,
// J[i][l] = E[phi_l(s_i Y)] with phi_l the hat functions of the piecewise-linear interpolant on the instance's s-grid (the last
// interval's two linear pieces continued beyond s_max), D the three-point central first-derivative stencil of hadi_fd_beta
// (the two-point backward difference at i = m1).  G depends on the s-grid and on (mu, sigma) only.
// MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's; the splitting is first order in time.
//
// hadi_jump_matrix_kernel builds G once per call in the operand order of the product kernel; hadi_jump_kernel is the product,
// on the matrix core (hadi_mfma_f64_16x16x4), out of place: it reads the copy of U that the caller put into UT and writes U.
// hadi_jump_sel_kernel is the same product (hadi_jump_step) for the nine groups of an eight-column Jacobian, which use three sets
// of matrices.
// Part of libhadi's device code: include through hadi_kernels.h (behind hadi_k_col.h).
#pragma once

#define HADI_JUMP_THREADS 256
#define HADI_JUMP_ROWS 64  // v-rows of one pass over the staged strip of G: one 16-row tile per wavefront
#define HADI_JUMP_KC 32    // slots of U per staged tile
#define HADI_JUMP_UP 34    // LDS pitch of a staged row of U: 16 rows x 2 k-columns of a half-wave fall on 32 different banks

// G in operand order.  Slots as the state's rows have them (hadi_pos), cut into blocks of 16 output slots and groups of 4 input
// slots; the K extent is padded to whole tiles of HADI_JUMP_KC slots.  Entry (output slot so, input slot sl) sits at
// ((so / 16) KG + sl / 4) 64 + 16 (sl % 4) + so % 16: the 64 doubles of one (block, group) are one B operand of the matrix
// instruction, lane by lane, and a block's strip is KG 64 contiguous doubles.  Pad slots and slots of nodes beyond m1 hold zeros.
HADI_HD inline int hadi_jump_kg(const HadiLayout &L) { return ((L.rowp + HADI_JUMP_KC - 1) / HADI_JUMP_KC) * (HADI_JUMP_KC / 4); }
HADI_HD inline int hadi_jump_nib(const HadiLayout &L) { return (L.rowp + 15) / 16; }
HADI_HD inline size_t hadi_jump_matrix_doubles(const HadiLayout &L) { return (size_t)hadi_jump_nib(L) * hadi_jump_kg(L) * 64; }
HADI_HD inline size_t hadi_jump_entry(int kg, int so, int sl) { return ((size_t)(so >> 4) * kg + (sl >> 2)) * 64 + 16 * (sl & 3) + (so & 15); }
HADI_HD inline size_t hadi_jump_smem(const HadiLayout &L) {
    return ((size_t)hadi_jump_kg(L) * 64 + (size_t)HADI_JUMP_ROWS * HADI_JUMP_UP) * sizeof(double);
}

// Phi(d1) - Phi(d0) for d0 <= d1, taken on the side of the smaller tail so that nothing cancels against 1.
HADI_HD inline double hadi_jump_dphi(double d0, double d1) {
    const double rs2 = 0.70710678118654752440;
    return d0 > 0.0 ? 0.5 * (erfc(d0 * rs2) - erfc(d1 * rs2)) : 0.5 * (erfc(-d1 * rs2) - erfc(-d0 * rs2));
}

// E[(a + b x) 1{x0 <= x < x1}] for x = s_i Y: a (Phi(d1) - Phi(d0)) + b s_i (1 + kbar) (Phi(d1 - sigma) - Phi(d0 - sigma)),
// d(x) = (ln(x / s_i) - mu) / sigma, Phi(d(0)) = 0, Phi(d(inf)) = 1.  to_inf: x1 is +inf.
HADI_HD inline double hadi_jump_piece(double a, double b, double x0, double x1, bool to_inf, double si, double mu, double sigma, double kb) {
    const double d0 = x0 > 0.0 ? (log(x0 / si) - mu) / sigma : -INFINITY;
    const double d1 = to_inf ? INFINITY : (log(x1 / si) - mu) / sigma;
    return a * hadi_jump_dphi(d0, d1) + b * si * (1.0 + kb) * hadi_jump_dphi(d0 - sigma, d1 - sigma);
}

// G[i][l] on the grid s[0 .. m1], i >= 1: the two intervals that touch node l, the identity, the compensator.
HADI_HD inline double hadi_jump_entry_value(const double *__restrict__ s, int m1, int i, int l, double mu, double sigma) {
    const double kb = exp(mu + 0.5 * sigma * sigma) - 1.0, si = s[i];
    double g = 0.0;
    if (l >= 1) {  // interval l - 1, where phi_l rises: (x - s_{l-1}) / h
        const double h = s[l] - s[l - 1];
        g += hadi_jump_piece(-s[l - 1] / h, 1.0 / h, s[l - 1], s[l], l == m1, si, mu, sigma, kb);
    }
    if (l <= m1 - 1) {  // interval l, where phi_l falls: (s_{l+1} - x) / h
        const double h = s[l + 1] - s[l];
        g += hadi_jump_piece(s[l + 1] / h, -1.0 / h, s[l], s[l + 1], l == m1 - 1, si, mu, sigma, kb);
    }
    if (l == i) g -= 1.0;
    double dw = 0.0;  // D[i][l]
    if (i < m1) {
        const double ha = s[i] - s[i - 1], hb = s[i + 1] - s[i];
        if (l == i - 1) dw = -hb / (ha * (ha + hb));
        else if (l == i) dw = (hb - ha) / (ha * hb);
        else if (l == i + 1) dw = ha / (hb * (ha + hb));
    } else {
        const double ha = s[m1] - s[m1 - 1];
        if (l == m1 - 1) dw = -1.0 / ha;
        else if (l == m1) dw = 1.0 / ha;
    }
    return g - kb * si * dw;
}

// Once per call, one thread per entry (i, l) of each of the n_mat matrices; matrix q is built on the s-grid of instance q
// (vec_s [..][m1 + 1]) with musig[2 q], musig[2 q + 1].  The caller has zeroed G: row 0, the pad slots and the K padding stay 0.
__global__ void __launch_bounds__(256) hadi_jump_matrix_kernel(HadiLayout L, int n_mat, const double *__restrict__ vec_s,
                                                               const double *__restrict__ musig, double *__restrict__ G) {
    const int m1p = L.m1 + 1;
    const size_t per = (size_t)m1p * m1p, e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per * (size_t)n_mat) return;
    const int q = (int)(e / per), i = (int)((e - (size_t)q * per) / m1p), l = (int)(e - (size_t)q * per - (size_t)i * m1p);
    if (i == 0) return;
    const double v = hadi_jump_entry_value(vec_s + (size_t)q * m1p, L.m1, i, l, musig[2 * q], musig[2 * q + 1]);
    G[(size_t)q * hadi_jump_matrix_doubles(L) + hadi_jump_entry(hadi_jump_kg(L), hadi_pos(L, i), hadi_pos(L, l))] = v;
}

// The natural-order copy of one matrix (hadi_debug_jump_matrix): out [m1 + 1][m1 + 1].
__global__ void __launch_bounds__(256) hadi_jump_matrix_unpack_kernel(HadiLayout L, const double *__restrict__ G, double *__restrict__ out) {
    const int m1p = L.m1 + 1;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m1p * m1p) return;
    const int i = (int)(e / m1p), l = (int)(e - (size_t)i * m1p);
    out[e] = G[hadi_jump_entry(hadi_jump_kg(L), hadi_pos(L, i), hadi_pos(L, l))];
}

// The caller's promise of a shared matrix: every row of vec_s [n][m1 + 1] is bit-equal to row 0.  A broken promise sets status[0].
__global__ void __launch_bounds__(256) hadi_jump_grid_check_kernel(int m1p, int n_inst, const double *__restrict__ vec_s, int *__restrict__ status) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)m1p * n_inst) return;
    const long long *b = reinterpret_cast<const long long *>(vec_s);
    if (b[e] != b[e % (size_t)m1p]) status[0] = 1;
}

// blocks: one per (group of ipg instances, block of 16 output slots); the blocks of an instance are neighbours in the grid, so
// that the copy of its U they all read stays in the caches while they run
// (rounded up to a multiple of 8 for hadi_xcd_remap: the surplus blocks return at once)
static inline unsigned hadi_jump_blocks(const HadiLayout &L, int n_inst, int ipg) { return (unsigned)((n_inst + ipg - 1) / ipg) * hadi_jump_nib(L); }
static inline unsigned hadi_jump_grid(const HadiLayout &L, int n_inst, int ipg) { return (hadi_jump_blocks(L, n_inst, ipg) + 7u) & ~7u; }

// The sub-step, streaming path, packed layout of any streaming shape (1, 2, 4, 8 nodes per lane, two wavefronts per row).
// U <- UT + a_k G UT per instance, UT the copy of U the caller made in front of this launch (out of place: every block of an
// instance reads all of the instance's old field, so nobody may overwrite it meanwhile).
// A block owns 16 output slots.  It stages its strip of G -- 16 rows, the whole K extent, already in operand order -- in LDS ONCE
// and keeps it for every v-row of every instance of its group that uses the same matrix (g_stride = 0: one matrix for the whole
// batch; else instance k of the batch uses matrix (inst0 + k) % n_src): G is read once per (matrix, step) from memory by the
// 16-slot blocks together, not once per strip of v-rows.  The v-rows go by in passes of 64, one 16 x 16 accumulator tile per
// wavefront; U comes through LDS in tiles of 64 rows x 32 slots, the loads of the next two tiles in flight while the matrix core
// works on this one (the re-reads of U are what the kernel waits for).  D = A B with A = the tile of U (lane 16 k + j: row j, slot k0 + k) and B = the strip of G transposed (lane
// 16 k + i: output slot i, input slot k0 + k), so register r of lane 16 q + i holds (row 4 r + q, output slot i): a wavefront
// stores 16 consecutive slots per row.
// Never written: pad slots, slots beyond m1, the identity rows past nrows.  Skipped, U bit-untouched: instances that have
// finished (n > N_k) and instances with a_k = 0.  The summation order over the input slots is the slot order, whatever the batch.
// The body is hadi_jump_step, for ngrp lists of instances: list_of(grp) names the instances of a block's list (start, stride,
// count; instances of the launch), mat_of(inst) the matrix of an instance as its offset into G, in doubles.  Which instances
// share a list never changes an instance's result.
struct HadiJumpList { int start, stride, count; };
template <class ListOf, class MatOf>
HADI_DEV HADI_FORCEINLINE void hadi_jump_step(double *smem, const HadiLayout &L, int ngrp, const double *__restrict__ UT,
                                              double *__restrict__ U, const double *__restrict__ G, const double *__restrict__ avec,
                                              const HadiInstPar *__restrict__ ipar, int n, ListOf list_of, MatOf mat_of) {
    const int kg = hadi_jump_kg(L), nib = hadi_jump_nib(L), rowp = L.rowp, nrows = L.nrows;
    double *const Gs = smem, *const Us = smem + (size_t)kg * 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The 16-slot blocks of an instance all read the instance's old field: consecutive logical ids go to ONE XCD, whose L2 then
    // holds that field (1.1 MB at 512x256) and the instance's matrix beside it.
    const int bid = hadi_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (bid >= ngrp * nib) return;  // (block-uniform: the padding of the grid)
    const int grp = bid / nib, ib = bid - grp * nib;
    const HadiJumpList li = list_of(grp);
    const int ntile = kg / (HADI_JUMP_KC / 4);
    // this thread's share of a tile of U: rows lr + 16 q (q < 4), the slot pair (kc + lc, kc + lc + 1)
    const int lr = tid >> 4, lc = 2 * (tid & 15);
    // what this lane owns of the result: rows 16 wave + 4 r + (lane >> 4), output slot so
    const int so = 16 * ib + (lane & 15), io = so < rowp ? hadi_slot_to_i(L, so) : -1;
    const bool so_ok = io >= 0 && io <= L.m1;
    long long cur = -1;  // the matrix whose strip is staged (its offset)
    for (int c = 0; c < li.count; c++) {
        const int inst = li.start + c * li.stride;
        const double a = avec[inst];
        if (a == 0.0 || n > ipar[inst].N) continue;  // (block-uniform)
        const long long mat = mat_of(inst);
        if (mat != cur) {
            __syncthreads();  // (nobody still reads the strip of the previous matrix)
            const double2 *__restrict__ src = reinterpret_cast<const double2 *>(G + mat + (size_t)ib * kg * 64);
            double2 *dst = reinterpret_cast<double2 *>(Gs);
            for (int e = tid; e < kg * 32; e += HADI_JUMP_THREADS) dst[e] = src[e];
            cur = mat;
        }
        const double *__restrict__ ut = UT + (size_t)inst * L.inst_stride;
        double *__restrict__ u = U + (size_t)inst * L.inst_stride;
        for (int j0 = 0; j0 < nrows; j0 += HADI_JUMP_ROWS) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            double2 nxa[4], nxb[4];  // two tiles ahead: the loads of tiles t + 1 and t + 2 are in flight while tile t is multiplied
            auto fetch = [&](int t, double2 (&nx)[4]) {  // tile t of U into registers: zeros past nrows, past the pitch and on slots that hold no node
                const int s0 = t * HADI_JUMP_KC + lc;
                const int i0 = s0 < rowp ? hadi_slot_to_i(L, s0) : -1, i1 = s0 + 1 < rowp ? hadi_slot_to_i(L, s0 + 1) : -1;
                const bool ok0 = i0 >= 0 && i0 <= L.m1, ok1 = i1 >= 0 && i1 <= L.m1;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = j0 + lr + 16 * q;
                    double2 v = double2{0.0, 0.0};
                    if (j < nrows && s0 < rowp) v = *reinterpret_cast<const double2 *>(ut + (size_t)j * rowp + s0);
                    nx[q] = double2{ok0 ? v.x : 0.0, ok1 ? v.y : 0.0};
                }
            };
            auto multiply = [&](int t, double2 (&nx)[4]) {  // tile t from its registers through LDS onto the matrix core
                __syncthreads();  // (the previous tile has been consumed; the first time: the strip of G may still be on its way)
#pragma unroll
                for (int q = 0; q < 4; q++) *reinterpret_cast<double2 *>(Us + (size_t)(lr + 16 * q) * HADI_JUMP_UP + lc) = nx[q];
                __syncthreads();
                if (t + 2 < ntile) fetch(t + 2, nx);
                const double *__restrict__ ap = Us + (size_t)(16 * wave + (lane & 15)) * HADI_JUMP_UP + (lane >> 4);
                const double *__restrict__ bp = Gs + (size_t)t * (HADI_JUMP_KC / 4) * 64 + lane;
#pragma unroll
                for (int kk = 0; kk < HADI_JUMP_KC / 4; kk++) hadi_mfma_f64_16x16x4(ap[4 * kk], bp[64 * kk], acc);
            };
            fetch(0, nxa);
            if (ntile > 1) fetch(1, nxb);
            for (int t = 0; t < ntile; t += 2) {
                multiply(t, nxa);
                if (t + 1 < ntile) multiply(t + 1, nxb);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = j0 + 16 * wave + 4 * r + (lane >> 4);
                if (so_ok && j < nrows) {
                    const size_t off = (size_t)j * rowp + so;
                    u[off] = ut[off] + a * acc[r];
                }
            }
        }
    }
}

// hadi_jump_kernel's lists: ipg consecutive instances each.
HADI_HD inline HadiJumpList hadi_jump_run(int n_inst, int ipg, int grp) {
    const int rest = n_inst - grp * ipg;
    return HadiJumpList{grp * ipg, 1, rest < ipg ? rest : ipg};
}

__global__ void __launch_bounds__(HADI_JUMP_THREADS) hadi_jump_kernel(HadiLayout L, int n_inst, int ipg, int inst0, int n_src,
                                                                      const double *__restrict__ UT, double *__restrict__ U,
                                                                      const double *__restrict__ G, long long g_stride,
                                                                      const double *__restrict__ avec,
                                                                      const HadiInstPar *__restrict__ ipar, int n) {
    HADI_DYN_SMEM(double, smem);
    hadi_jump_step(smem, L, (n_inst + ipg - 1) / ipg, UT, U, G, avec, ipar, n, [=](int grp) { return hadi_jump_run(n_inst, ipg, grp); },
                   [=](int inst) { return g_stride ? (long long)((inst0 + inst) % n_src) * g_stride : 0ll; });
}

// ---- the nine groups of an eight-column Jacobian (hadi_compute_jacobian_bates_jumps) --------------------------------------------
// The batch is 9 groups of n_src source instances, instance k = group k / n_src, source k % n_src.  The groups 0 .. 6 (base, kappa,
// eta, sigma, rho, V_0, lambda) use the matrices of (mu, sigma), group 7 those of (mu + eps, sigma), group 8 those of (mu, sigma +
// eps): three sets of `per` matrices, G [3][per], per = n_src (one matrix per source instance and set) or 1 (one per set, shared by
// the batch).
#define HADI_JUMP_GROUPS 9
#define HADI_JUMP_SETS 3
HADI_HD inline int hadi_jump_set(int g) { return g <= 6 ? 0 : g - 6; }
// A launch covers the instances inst0 .. inst0 + n_inst of the batch (a sub-batch).  share = 0: the lists are cap consecutive
// instances, as hadi_jump_kernel's.  share = 1 (per = n_src only): the instances of ONE source instance that fall into the launch
// and use the same matrix ride on one staged strip -- source `t` of the launch's first min(n_inst, n_src) instances owns
// nq = ceil(7 / cap) + 2 lists: its set-0 instances t, t + n_src, ... in chunks of cap, then its group-7 and its group-8 instance
// (a list may be empty: its blocks return at once).
struct HadiJumpSel { int inst0, n_src, per, share, cap; };
HADI_HD inline int hadi_jump_sel_nq(const HadiJumpSel &q) { return (7 + q.cap - 1) / q.cap + 2; }
HADI_HD inline int hadi_jump_sel_ngrp(const HadiJumpSel &q, int n_inst) {
    if (!q.share) return (n_inst + q.cap - 1) / q.cap;
    return (n_inst < q.n_src ? n_inst : q.n_src) * hadi_jump_sel_nq(q);
}
HADI_HD inline HadiJumpList hadi_jump_sel_list(const HadiJumpSel &q, int n_inst, int grp) {
    if (!q.share) return hadi_jump_run(n_inst, q.cap, grp);
    const int nq = hadi_jump_sel_nq(q), t = grp / nq, slot = grp - t * nq;
    const int g0 = (q.inst0 + t) / q.n_src;                // the group of the owner's first instance of the launch
    const int C = (n_inst - t + q.n_src - 1) / q.n_src;    // its instances in the launch: groups g0 .. g0 + C - 1
    int c0 = 7 - g0;                                       // ... of which the first c0 are of set 0
    c0 = c0 < 0 ? 0 : (c0 > C ? C : c0);
    if (slot < nq - 2) {
        const int rest = c0 - slot * q.cap;
        return HadiJumpList{t + slot * q.cap * q.n_src, q.n_src, rest < 0 ? 0 : (rest < q.cap ? rest : q.cap)};
    }
    const int c = (slot == nq - 2 ? 7 : 8) - g0;
    return HadiJumpList{t + c * q.n_src, q.n_src, (c >= 0 && c < C) ? 1 : 0};
}
static inline unsigned hadi_jump_sel_grid(const HadiLayout &L, const HadiJumpSel &q, int n_inst) {
    return ((unsigned)hadi_jump_sel_ngrp(q, n_inst) * hadi_jump_nib(L) + 7u) & ~7u;
}

// hadi_jump_kernel for such a batch: instance inst0 + inst uses matrix hadi_jump_set(group) * per + (per > 1 ? source : 0).  Per
// instance the arithmetic and the summation order are hadi_jump_kernel's: the two share hadi_jump_step.
__global__ void __launch_bounds__(HADI_JUMP_THREADS) hadi_jump_sel_kernel(HadiLayout L, int n_inst, HadiJumpSel q,
                                                                          const double *__restrict__ UT, double *__restrict__ U,
                                                                          const double *__restrict__ G, long long g_stride,
                                                                          const double *__restrict__ avec,
                                                                          const HadiInstPar *__restrict__ ipar, int n) {
    HADI_DYN_SMEM(double, smem);
    hadi_jump_step(smem, L, hadi_jump_sel_ngrp(q, n_inst), UT, U, G, avec, ipar, n,
                   [=](int grp) { return hadi_jump_sel_list(q, n_inst, grp); },
                   [=](int inst) {
                       const int k = q.inst0 + inst, g = k / q.n_src;
                       return (long long)(hadi_jump_set(g) * q.per + (q.per > 1 ? k - g * q.n_src : 0)) * g_stride;
                   });
}
