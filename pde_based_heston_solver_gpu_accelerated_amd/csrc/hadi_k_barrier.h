// hadi_k_barrier.h -- discretely monitored knock-out barriers: after the last pass of a monitoring step every node (i, j) of the
// instances that list the step takes U <- rebate where its spot node is at or beyond a barrier (s_i <= lower or s_i >= upper:
// touching knocks out), every v-row alike.  The rebate is paid at the knock-out: nothing is discounted.
// MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's (the Dirichlet edge at s_max and the v-edge rows
// carry the vanilla time factors); the knock-out overwrites the knocked nodes -- those edges among them -- on monitoring steps
// only, and between two monitoring dates the option is alive everywhere, as a discretely monitored contract is.
// hadi_barrier_locate_kernel turns the two comparisons into the index range (ia, ib) of the live nodes once per call; the
// whole-loop kernels knock their LDS field (hadi_knock_lds), the streaming path launches hadi_knockout_kernel between two steps.
// Both compare indices only.  The monitoring table has the shape of the Bermudan exercise table and is read with hadi_ex_listed.
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// Once per call, one thread per instance: iab[2k], iab[2k+1] = first and last index i with lower_k < s_i < upper_k on the
// instance's own s-grid; (m1 + 1, -1) -- ia > ib -- when no node is alive.  bounds[2k], bounds[2k+1] = lower_k, upper_k
// (-inf / +inf = no barrier on that side).  THE one place that decides <= / >=.
__global__ void __launch_bounds__(64) hadi_barrier_locate_kernel(HadiLayout L, int n_inst, const double *__restrict__ vec_s,
                                                                 const double *__restrict__ bounds, int *__restrict__ iab) {
    const int inst = blockIdx.x * blockDim.x + threadIdx.x;
    if (inst >= n_inst) return;
    const double *s = vec_s + (size_t)inst * (L.m1 + 1);
    const double lower = bounds[2 * (size_t)inst], upper = bounds[2 * (size_t)inst + 1];
    int ia = L.m1 + 1, ib = -1;
    for (int i = 0; i <= L.m1; i++) {
        const bool knocked = s[i] <= lower || s[i] >= upper;
        if (!knocked) {
            if (i < ia) ia = i;
            ib = i;
        }
    }
    iab[2 * (size_t)inst] = ia;
    iab[2 * (size_t)inst + 1] = ib;
}

HADI_HD inline bool hadi_knocked(int i, int ia, int ib) { return i < ia || i > ib; }

// Whole-loop kernels: the instance's field lives in LDS, in the packed order (natural = false) or in natural order (the
// sequential kernels), with pitch `pitch`.  Thread t of nt; the caller puts a barrier on either side.  Only nodes are touched:
// pad slots stay.  Nothing is read.
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_knock_lds(double *Ul, int pitch, bool natural, int ia, int ib, double rebate, int nrows, int m1,
                                              int t, int nt) {
    for (int e = t; e < nrows * (m1 + 1); e += nt) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        if (hadi_knocked(i, ia, ib)) Ul[(size_t)j * pitch + (natural ? i : hadi_pos(B, 1, i))] = rebate;
    }
}

// Streaming path, packed layout of any shape (1, 2, 4, 8 nodes per lane, two wavefronts per row, the sequential passes' natural
// rows).  Blocks map to instances -- bpi blocks each (hadi_exercise_bpi) -- so the per-instance flag is block-uniform and an
// instance that does not list the step returns at once.  A pair with both nodes alive costs no memory access; a pair with both
// knocked is one 16-byte store; a mixed pair stores its knocked node only.  Pad slots, slots of nodes beyond m1 and the identity
// rows past nrows are never written.  At most 8 B per knocked node, nothing read.
__global__ void __launch_bounds__(HADI_EX_THREADS) hadi_knockout_kernel(HadiLayout L, int n_inst, int bpi, double *__restrict__ U,
                                                                         const int *__restrict__ mon_flag, int mon_stride,
                                                                         const int *__restrict__ iab, const double *__restrict__ rebate,
                                                                         int n) {
    const int inst = (int)(blockIdx.x / (unsigned)bpi), b = (int)(blockIdx.x - (unsigned)inst * (unsigned)bpi);
    if (inst >= n_inst || !hadi_ex_listed(mon_flag, mon_stride, inst, n)) return;
    const int ia = iab[2 * (size_t)inst], ib = iab[2 * (size_t)inst + 1];
    if (ia == 0 && ib == L.m1) return;  // (both barriers outside the grid)
    const double reb = rebate[inst];
    const int hp = L.rowp >> 1, npairs = L.nrows * hp;
    double *__restrict__ u = U + (size_t)inst * L.inst_stride;
    double2 *__restrict__ u2 = reinterpret_cast<double2 *>(u);
    for (int e = b * HADI_EX_THREADS + (int)threadIdx.x; e < npairs; e += bpi * HADI_EX_THREADS) {
        const int j = e / hp, slot = 2 * (e - j * hp);
        const int i0 = hadi_slot_to_i(L, slot), i1 = hadi_slot_to_i(L, slot + 1);
        const bool k0 = i0 >= 0 && i0 <= L.m1 && hadi_knocked(i0, ia, ib), k1 = i1 >= 0 && i1 <= L.m1 && hadi_knocked(i1, ia, ib);
        if (k0 && k1) u2[e] = double2{reb, reb};
        else if (k0) u[2 * (size_t)e] = reb;
        else if (k1) u[2 * (size_t)e + 1] = reb;
    }
}
