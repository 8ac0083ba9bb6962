// hadi_k_bermudan.h -- Bermudan exercise: U <- max(U, payoff) on every node of the instances that list the step, after the step's
// last pass.  The whole-loop kernels apply it to their LDS field (hadi_exercise_lds); the streaming path launches
// hadi_exercise_kernel between two steps.
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// The exercise table (host-built, as the dividend table): ex_flag[k * ex_stride + n - 1] != 0 = instance k may be exercised at
// the END of step n; ex_stride 0 = one shared row.  nullptr = no exercise at all.
HADI_HD inline bool hadi_ex_listed(const int *ex_flag, int ex_stride, int inst, int n) {
    return ex_flag && ex_flag[(size_t)inst * ex_stride + n - 1] != 0;
}

// Whole-loop kernels: the instance's field lives in LDS, in the packed order with pitch rowp (natural = false) or in natural
// order with pitch `pitch` (the sequential kernels); the payoff is read from the instance's packed global array P0g, on
// exercise steps only.  Thread t of nt; the caller puts a barrier on either side.  Only nodes are touched: pad slots stay.
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_exercise_lds(double *Ul, int pitch, bool natural, const double *__restrict__ P0g, int nrows, int m1,
                                                 int rowp, int t, int nt) {
    for (int e = t; e < nrows * (m1 + 1); e += nt) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        const int slot = hadi_pos(B, 1, i);
        double *u = Ul + (size_t)j * pitch + (natural ? i : slot);
        *u = fmax(*u, P0g[(size_t)j * rowp + slot]);
    }
}

// Streaming path, packed layout of any shape (1, 2, 4, 8 nodes per lane, two wavefronts per row, the sequential passes' natural
// rows).  Blocks map to instances -- bpi blocks each -- so the per-instance flag is block-uniform and an unlisted instance
// returns at once.  Rows start on 64-byte boundaries and rowp is even: 16-byte accesses, 24 B per point (U read and written, the
// payoff read).  A pair's slots are tested one by one: pad slots (and slots of nodes beyond m1) keep their value.
#define HADI_EX_THREADS 256
__global__ void __launch_bounds__(HADI_EX_THREADS) hadi_exercise_kernel(HadiLayout L, int n_inst, int bpi, double *__restrict__ U,
                                                                         const double *__restrict__ P0, const int *__restrict__ ex_flag,
                                                                         int ex_stride, int n) {
    const int inst = (int)(blockIdx.x / (unsigned)bpi), b = (int)(blockIdx.x - (unsigned)inst * (unsigned)bpi);
    if (inst >= n_inst || !hadi_ex_listed(ex_flag, ex_stride, inst, n)) return;
    const int hp = L.rowp >> 1, npairs = L.nrows * hp;  // (v-rows past nrows are identity rows: always 0, never touched)
    double2 *__restrict__ u2 = reinterpret_cast<double2 *>(U + (size_t)inst * L.inst_stride);
    const double2 *__restrict__ p2 = reinterpret_cast<const double2 *>(P0 + (size_t)inst * L.inst_stride);
    for (int e = b * HADI_EX_THREADS + (int)threadIdx.x; e < npairs; e += bpi * HADI_EX_THREADS) {
        const int j = e / hp, slot = 2 * (e - j * hp);
        const int i0 = hadi_slot_to_i(L, slot), i1 = hadi_slot_to_i(L, slot + 1);
        const bool k0 = i0 >= 0 && i0 <= L.m1, k1 = i1 >= 0 && i1 <= L.m1;
        if (!k0 && !k1) continue;
        double2 u = u2[e];
        const double2 p = p2[e];
        if (k0) u.x = fmax(u.x, p.x);
        if (k1) u.y = fmax(u.y, p.y);
        u2[e] = u;
    }
}
// blocks per instance: one per HADI_EX_THREADS pairs, at most 64 (a 512x256 instance has 66 820 pairs: four trips)
static inline int hadi_exercise_bpi(const HadiLayout &L) {
    const int npairs = L.nrows * (L.rowp >> 1), want = (npairs + HADI_EX_THREADS - 1) / HADI_EX_THREADS;
    return want < 1 ? 1 : want > 64 ? 64 : want;
}
