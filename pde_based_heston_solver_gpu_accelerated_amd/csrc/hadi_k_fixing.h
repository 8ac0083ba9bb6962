// hadi_k_fixing.h -- strike fixings of forward-start options and cliquets: after the last pass of a fixing step every node (i, j) of
// the instances that list the step takes
//     c_j     = U(i_ref, j)                    read before anything of the event is written
//     U(i, j) <- a_i * c_j + w * P(i, j)       the term w * P only when w != 0
// on every v-row, boundary rows included.  i_ref is the node of the instance's reference spot; a_i = s_i / s_{i_ref}
// (HADI_FIXM_SHARES: the strike is proportional to the fixing spot, a_{i_ref} is exactly 1) or a_i = 1 (HADI_FIXM_RETURN: the row
// becomes flat); w is the weight of that fixing date and P the packed payoff field of the Bermudan calls.
// MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's, as for barriers.
// Unlike the exercise and the knock-out, which read and write the same slot, every node of a v-row reads ONE node of the row and is
// then overwritten, the source node included.  The whole-loop kernels (hadi_fixing_lds) write every column but i_ref, synchronise,
// and then do column i_ref; the streaming path has no block-wide order across the blocks of an instance and takes two stream-ordered
// launches: hadi_fixing_gather_kernel copies c_j out, hadi_fixing_kernel applies the event from the copy.
// With w == 0 the SHARES event leaves node (i_ref, j) with its bits and the RETURN event leaves every node of row j with c_j's bits:
// a factor of exactly 1 is never multiplied in, and no w * P term is formed.
// The fixing table has the shape of the Bermudan exercise table and is read with hadi_ex_listed; the weights' table has the same
// shape and stride.  Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

enum { HADI_FIXM_SHARES = 0, HADI_FIXM_RETURN = 1 };  // enum hadi_fixing_mode (static_assert in hadi_api.hip)

// Once per call, one thread per instance: i_ref[k] = the first node of the instance's own s-grid within 1e-10 of ref_spot[k] (the
// price pick's rule), or -1 and status[k] = 1 when there is none.  THE one place that applies the 1e-10 rule.
__global__ void __launch_bounds__(64) hadi_fixing_locate_kernel(HadiLayout L, int n_inst, const double *__restrict__ vec_s,
                                                                const double *__restrict__ ref_spot, int *__restrict__ i_ref,
                                                                int *__restrict__ status) {
    const int inst = blockIdx.x * blockDim.x + threadIdx.x;
    if (inst >= n_inst) return;
    const double *s = vec_s + (size_t)inst * (L.m1 + 1);
    const double x = ref_spot[inst];
    int is = -1;
    for (int i = 0; i <= L.m1; i++)
        if (fabs(s[i] - x) < 1e-10) { is = i; break; }
    i_ref[inst] = is;
    status[inst] = is < 0 ? 1 : 0;
}

// a_i * c for a node other than i_ref (sref = s_{i_ref}).
HADI_HD inline double hadi_fix_scaled(int mode, double si, double sref, double c) { return mode == HADI_FIXM_RETURN ? c : (si / sref) * c; }

// Whole-loop kernels: the instance's field lives in LDS, in the packed order (natural = false) or in natural order (the
// sequential kernels), with pitch `pitch`; the payoff is read from the instance's packed global array P0g (pitch rowp), only where
// w != 0; vs is the instance's s-grid.  Thread t of nt; the caller puts a barrier on either side, and every thread of the block
// comes here (the barrier inside).  Phase 1 writes every column but ir -- so column ir still holds c_j for every reader --, phase 2,
// behind the barrier, adds w * P to column ir (a_{ir} = 1: with w == 0 the column keeps its bits).  Only nodes are touched: pad
// slots stay.  ir < 0 (the reference spot is off the grid: the call fails) leaves the field alone.
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_fixing_lds(double *Ul, int pitch, bool natural, const double *__restrict__ P0g,
                                               const double *__restrict__ vs, int ir, int mode, double w, int nrows, int m1, int rowp,
                                               int t, int nt) {
    if (ir < 0) return;  // (uniform over the instance's threads)
    const int sref_slot = hadi_pos(B, 1, ir), pref = natural ? ir : sref_slot;
    const double sref = vs[ir];
    for (int e = t; e < nrows * (m1 + 1); e += nt) {
        const int j = e / (m1 + 1), i = e - j * (m1 + 1);
        if (i == ir) continue;
        const int slot = hadi_pos(B, 1, i);
        double val = hadi_fix_scaled(mode, vs[i], sref, Ul[(size_t)j * pitch + pref]);
        if (w != 0.0) val += w * P0g[(size_t)j * rowp + slot];
        Ul[(size_t)j * pitch + (natural ? i : slot)] = val;
    }
    __syncthreads();
    if (w != 0.0)
        for (int j = t; j < nrows; j += nt) Ul[(size_t)j * pitch + pref] += w * P0g[(size_t)j * rowp + sref_slot];
}

// The weight of step n for instance `inst` (nullptr: all weights are 0).
HADI_HD inline double hadi_fix_weight(const double *fix_w, int fix_stride, int inst, int n) {
    return fix_w ? fix_w[(size_t)inst * fix_stride + n - 1] : 0.0;
}

// Streaming path, first launch of a fixing step: c[inst * c_stride + j] = U(i_ref, j) for the instances that list step n, one
// thread per (instance, v-row).  c_stride >= nrows.
__global__ void __launch_bounds__(256) hadi_fixing_gather_kernel(HadiLayout L, int n_inst, const double *__restrict__ U,
                                                                 const int *__restrict__ fix_flag, int fix_stride,
                                                                 const int *__restrict__ i_ref, double *__restrict__ c, int c_stride, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int inst = e / L.nrows, j = e - inst * L.nrows;
    if (inst >= n_inst || !hadi_ex_listed(fix_flag, fix_stride, inst, n)) return;
    const int ir = i_ref[inst];
    if (ir < 0) return;
    c[(size_t)inst * c_stride + j] = U[(size_t)inst * L.inst_stride + (size_t)j * L.rowp + hadi_pos(L, ir)];
}

// Streaming path, second launch: the event from the gathered c, packed layout of any shape (1, 2, 4, 8 nodes per lane, two
// wavefronts per row, the sequential passes' natural rows).  The shape of hadi_knockout_kernel: blocks map to instances -- bpi
// blocks each (hadi_exercise_bpi) -- so the per-instance flag is block-uniform and an instance that does not list the step returns
// at once; 16-byte pairs through hadi_slot_to_i; pad slots, slots of nodes beyond m1 and the identity rows past nrows are never
// written.  8 B written per node, 8 B read from the packed payoff only where w != 0; a_i from the instance's vec_s.
__global__ void __launch_bounds__(HADI_EX_THREADS) hadi_fixing_kernel(HadiLayout L, int n_inst, int bpi, double *__restrict__ U,
                                                                       const double *__restrict__ P0, const int *__restrict__ fix_flag,
                                                                       const double *__restrict__ fix_w, int fix_stride,
                                                                       const int *__restrict__ i_ref, const int *__restrict__ mode_i,
                                                                       const double *__restrict__ c, int c_stride,
                                                                       const double *__restrict__ vec_s, int n) {
    const int inst = (int)(blockIdx.x / (unsigned)bpi), b = (int)(blockIdx.x - (unsigned)inst * (unsigned)bpi);
    if (inst >= n_inst || !hadi_ex_listed(fix_flag, fix_stride, inst, n)) return;
    const int ir = i_ref[inst];
    if (ir < 0) return;
    const int mode = mode_i[inst];
    const double w = hadi_fix_weight(fix_w, fix_stride, inst, n);
    const double *__restrict__ s = vec_s + (size_t)inst * (L.m1 + 1);
    const double sref = s[ir];
    const double *__restrict__ ci = c + (size_t)inst * c_stride;
    const int hp = L.rowp >> 1, npairs = L.nrows * hp;
    double *__restrict__ u = U + (size_t)inst * L.inst_stride;
    double2 *__restrict__ u2 = reinterpret_cast<double2 *>(u);
    const double2 *__restrict__ p2 = reinterpret_cast<const double2 *>(P0 + (size_t)inst * L.inst_stride);
    for (int e = b * HADI_EX_THREADS + (int)threadIdx.x; e < npairs; e += bpi * HADI_EX_THREADS) {
        const int j = e / hp, slot = 2 * (e - j * hp);
        const int i0 = hadi_slot_to_i(L, slot), i1 = hadi_slot_to_i(L, slot + 1);
        const bool k0 = i0 >= 0 && i0 <= L.m1, k1 = i1 >= 0 && i1 <= L.m1;
        if (!k0 && !k1) continue;
        const double cj = ci[j];
        double x0 = !k0 || i0 == ir ? cj : hadi_fix_scaled(mode, s[i0], sref, cj);
        double x1 = !k1 || i1 == ir ? cj : hadi_fix_scaled(mode, s[i1], sref, cj);
        if (w != 0.0) {
            const double2 p = p2[e];
            x0 += w * p.x;
            x1 += w * p.y;
        }
        if (k0 && k1) u2[e] = double2{x0, x1};
        else if (k0) u[2 * (size_t)e] = x0;
        else u[2 * (size_t)e + 1] = x1;
    }
}
