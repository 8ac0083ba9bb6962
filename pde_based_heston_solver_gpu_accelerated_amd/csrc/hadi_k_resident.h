// hadi_k_resident.h -- one launch per batch for European Douglas sweeps on strips of one block per instance (hadi_sweep_resident).
// Part of libhadi's device code: include through hadi_kernels.h (which fixes the order).
#pragma once

// ------------------------------------------------------------------------------------------------
// Resident sweep.  Where the plan runs the row pass of every instance as ONE strip block (8 nodes per lane, one wavefront per
// v-row, sblocks = 1) and the batch fills at most one round of CUs, the two passes of a step depend on each other only inside
// an instance -- and an instance is one workgroup.  So one block per instance runs the whole time loop:
//   row phase     the body of hadi_pass_a_strip<B, EU> (hadi_k_row_strip_body.h: the same source, the same template arguments,
//                 the same counted waits), included into a function so that its early returns end the phase, not the kernel;
//   drain         every wavefront retires its stores (s_waitcnt vmcnt(0)), then __syncthreads(): the readers of Y are the
//                 other wavefronts of the same CU, behind the same vector L1 (workgroup scope, no invalidate, no grid barrier);
//   column phase  every column tile of the instance with the hadi_pb_* functions of hadi_pass_b<8, EU> (chunk sweeps, the
//                 reduced system on the matrix core, three register buffers), its LDS aliasing the row phase's rings;
//   drain.
// What goes away against the streaming path: two dependent kernel boundaries per step, the column pass's three rounds of
// blocks (each paying for its first tile's loads) and the chip-wide prologue burst at the start of every pass.
// LDS: [8 rings of 4 rows][4 s-coefficient arrays] as in hadi_pass_a_strip, [RT: the column phase's selected inverse rows]
// behind them (hadi_resident_smem); the column phase's exchange values Z and the product T alias the first two rings.
//
// Phase boundaries.  What does not depend on the step is staged by the block's FIRST step only and stays in LDS that no ring
// aliases: the s-coefficient arrays (row phase) and RT (column phase).  Each boundary is two separate points -- "my stores have
// retired" (hadi_resident_retire: the wavefront's own s_waitcnt vmcnt(0)) and "the block has met" (__syncthreads) -- and the
// column phase issues between them what needs no other wavefront: its chunk table (no step writes it) and, where every
// wavefront owns the same v-rows in both phases (a.RS == HADI_LC, a.sblocks == 1: strip w = rows [33 w, 33 w + 33) = chunk w),
// the loads of its first two column tiles, which are rows it stored itself.  The short column tile runs second, not last: its
// solve moves almost no memory and now overlaps the full tiles' traffic instead of standing alone in front of the drain.

// Registers.  Either phase alone sits at ~250 VGPRs.  Around the time loop hipcc hoists what each phase derives from the thread
// index (lane offsets, the column table's lane -> entry map) and the kernel arguments out of the loop, so all of it stays
// live through the OTHER phase too: 256 VGPRs with 31 spilled and scratch reloads inside the row loop.  Both phases therefore
// see the thread index through an empty asm (a local `threadIdx` that shadows the builtin inside the phase) and take the
// argument block from a fresh load of the kernarg segment: what they derive is recomputed every step, a few scalar and
// integer instructions per phase (254 VGPRs, nothing spilled).
HADI_DEV HADI_FORCEINLINE unsigned hadi_resident_tid() {
#if defined(HADI_EMU)
    return threadIdx.x;
#else
    unsigned t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
#endif
}
#if defined(HADI_EMU)
#define HADI_RESIDENT_TID
#else
#define HADI_RESIDENT_TID const struct { unsigned x; } threadIdx = {hadi_resident_tid()};
#endif

// The kernel's argument block, loaded again from the kernarg segment (scalar loads; `a` is the kernel's first parameter, at
// offset 0) behind an empty asm: see "Registers" above.
HADI_DEV HADI_FORCEINLINE HadiSweepArgs hadi_resident_args(const HadiSweepArgs &a) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)a;
    typedef const __attribute__((address_space(4))) HadiSweepArgs *HadiKargPtr;
    HadiKargPtr p = (HadiKargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *p;
#else
    return a;  // (host pass and emulator)
#endif
}

// Diagnostic build only (-DHADI_STAMPS=5, tools/resident_stamps.py): shader-clock cycles of the pieces of a resident step, summed per
// wavefront in the last KiB of the CU's LDS (lane 0; slot 15 = the previous stamp) and added to g_hadi_stamps at the kernel's end.
//   0 row prologue (to its second barrier)  1 row loop  2 retire + meet  3 column prologue  4 full tiles  5 short tile  6 final drain
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
#define HADI_RES_STAMP_LDS_BYTES 163840
HADI_DEV HADI_FORCEINLINE void hadi_res_stamp(int k) {  // k < 0: only starts the clock
    if (HADI_STAMPS != 5) return;
    HADI_DYN_SMEM(unsigned long long, s);
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *w = s + (HADI_RES_STAMP_LDS_BYTES - 1024) / 8 + (threadIdx.x >> 6) * 16;
        if (k >= 0) w[k] += t - w[15];
        w[15] = t;
    }
}
#define HADI_RES_STAMP(k) hadi_res_stamp(k)
#else
#define HADI_RES_STAMP(k)
#endif

// Row phase: hadi_pass_a_strip<B, 0, double, 1, 0> for step n.  `first`: the block's first step stages the coefficient arrays.
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_resident_row_phase(const HadiSweepArgs &a, int n, bool first) {
    HADI_RESIDENT_TID
    constexpr int AMER = 0, G = 1, MODE = 0, SCH = HADI_SCH_CS;
    typedef double T;
#define HADI_BODY_RESTAGE first
#include "hadi_k_row_strip_body.h"
#undef HADI_BODY_RESTAGE
}

// This wavefront's loads and stores have retired: its Y / U rows are in the CU's L1 and L2, where the other wavefronts of the
// block -- the same CU, the same vector L1 -- and this one read them (workgroup scope, no invalidate, no grid barrier).
HADI_DEV HADI_FORCEINLINE void hadi_resident_retire() {
#if !defined(HADI_EMU)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

// Column phase: the European branch of hadi_pass_b<8, 0, double> with ONE block per instance -- all ctiles tiles.  Entered by
// every wavefront behind its own hadi_resident_retire(); the block meets INSIDE (once, every wavefront).  Wavefronts without a
// chunk (P < 8) only take part in that meeting and in the block barriers of every tile's reduced system.
HADI_DEV HADI_FORCEINLINE void hadi_resident_col_phase(const HadiSweepArgs &a, int inst, bool first) {
    HADI_DYN_SMEM(double, smem);
    HADI_RESIDENT_TID
    HadiPassBCtx c;
    c.lane = threadIdx.x & 63;
    c.wave = HADI_UNIFORM((int)(threadIdx.x >> 6));
    c.P = a.L.P;
    const int P = c.P, cnt = a.ctiles;
    if (c.wave >= P) {
        __syncthreads();  // (the block meets: the row phase is over)
        if (P > 1) {
            for (int t = 0; t < cnt; t++) {
                __syncthreads();
                if (HADI_PB_MF) __syncthreads();
            }
        }
        return;
    }
    const HadiInstPar ip = a.ipar[inst];
    c.nrows = a.L.nrows;
    c.rowp = a.L.rowp;
    c.ja = c.wave * HADI_LC;
    c.Yi = a.Y + (size_t)inst * a.L.inst_stride;
    c.Ui = a.U + (size_t)inst * a.L.inst_stride;
    c.Yb = hadi_make_buf(c.Yi, (size_t)a.L.inst_stride * sizeof(double));
    c.Ub = hadi_make_buf(c.Ui, (size_t)a.L.inst_stride * sizeof(double));
    c.Li = nullptr; c.Lb = hadi_make_buf(nullptr, 0); c.P0i = nullptr; c.pay1d = 0;
    c.american = 0; c.debug = a.debug;
    c.pos_m1 = a.pos_m1;
    c.tabl = nullptr;
    // Tile order: the first full tile, the SHORT one, then the other full tiles.  Tiles are independent; only the order of the
    // three-buffer rotation changes.
    // cnt == nfull + 1 always: the pitch is 64 B G + pad, so the last tile is a short one (see hadi_pb_tiles in hadi_k_col.h, and
    // hadi_plan.h, which sets ctiles); a block whose argument block said otherwise keeps the plain order.
    const int nfull = a.L.rowp >> 6;
    const bool short_second = cnt == nfull + 1 && cnt >= 3;  // (block-uniform)
    auto tile = [&](int i) {
        if (!short_second || i == 0) return i;
        return i == 1 ? nfull : i - 1;
    };
    // Column LDS: [Z: 4 P x 64][T: MP x 64] on the first two rings; RT behind the row phase's coefficient arrays, where
    // it survives the row phase: staged by the first step alone.  No barrier of its own: every tile's reduced system reads RT
    // behind the barrier that follows the tile's exchange writes, which every staging wavefront reaches after its RT stores.
    static_assert(HADI_PB_MF != 0, "the resident column phase has the matrix-core LDS layout only (no Ri rows)");
    const int n4 = 4 * P, MP = hadi_pb_mp(P);
    c.zsh = smem; c.Ri = nullptr;
    c.Tsh = smem + (size_t)n4 * 64;
    double *const RT = smem + hadi_resident_rt_offset(a.L);
    c.RT = RT;
    // (block-uniform) every wavefront's chunk rows are the rows of its own strip: see "Phase boundaries" above
    const bool own = a.RS == HADI_LC && a.sblocks == 1;
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    unsigned long long stamp_store_[32] = {0};  // (the hadi_pb_* functions' own stamps, HADI_STAMPS=3: summed nowhere here)
    c.stamp_acc_ = stamp_store_;
#endif
    double ya[HADI_LC], yb[HADI_LC], yc[HADI_LC];
    // ---- independent of the row phase: requested while the slower wavefronts still finish their strips ----
    hadi_pb_load_table(c, a.pb + ((size_t)inst * a.L.nrows_pad + c.ja) * HADI_PBW);
    if (first) hadi_pb_stage_rt(a.rinv + (size_t)inst * 16 * P * P, P, RT, 64 * P);
    // The block meets BEFORE the tile loads where they read rows of other wavefronts, BEHIND them where they are this wavefront's
    // own (one site per load).  Nothing above or between writes ring-aliased LDS: the first such write is the exchange of the
    // first solve, behind the meeting either way -- every wavefront has then left its row loop (its ring reads retired by the
    // loop's own lgkmcnt(0), its LDS-DMA by hadi_resident_retire()).
    if (!own) __syncthreads();
    hadi_pb_load<double>(c, tile(0), ya);
    if (1 < cnt) hadi_pb_load<double>(c, tile(1), yb);
    if (own) __syncthreads();
    HADI_RES_STAMP(2);  // retire + meet
    c.inv_dt = 1.0 / ip.dt;
    c.dt = ip.dt;
    HADI_RES_STAMP(3);  // column prologue
    for (int i = 0; i < cnt; i += 3) {
        if (i + 2 < cnt) hadi_pb_load<double>(c, tile(i + 2), yc);
        hadi_pb_solve_store<0, double>(c, tile(i), i & 1, ya, 0);
        HADI_RES_STAMP(tile(i) == nfull ? 5 : 4);
        if (i + 1 < cnt) {
            if (i + 3 < cnt) hadi_pb_load<double>(c, tile(i + 3), ya);
            hadi_pb_solve_store<0, double>(c, tile(i + 1), (i + 1) & 1, yb, 0);
            HADI_RES_STAMP(tile(i + 1) == nfull ? 5 : 4);
        }
        if (i + 2 < cnt) {
            if (i + 4 < cnt) hadi_pb_load<double>(c, tile(i + 4), yb);
            hadi_pb_solve_store<0, double>(c, tile(i + 2), (i + 2) & 1, yc, 0);
            HADI_RES_STAMP(tile(i + 2) == nfull ? 5 : 4);
        }
    }
}

// Grid: the sub-batch's instances, padded to a multiple of 8 (the strip body's XCD remap: logical block = instance).
// N: the sweep's step count; an instance with fewer steps (per-instance maturities) stops at its own.
// `a` MUST stay the first parameter: hadi_resident_args() reads the argument block at offset 0 of the kernarg segment
// (tests/test_isa_resident.py checks that the kernel's metadata puts it there).
// Barriers: every wavefront of a block runs the same Ni steps (Ni is block-uniform, and the phase bodies' `n > ip.N` returns
// cannot be taken below it), and per step it meets the block at the row prologue's two barriers (in front of the body's
// `!has_strip` return), once inside the column phase, at the two barriers of every column tile (the idle wavefronts' loop
// counts the same tiles) and at the step's end.
template <int B>
__global__ void __launch_bounds__(64 * HADI_STRIP_WAVES(B), 2) hadi_sweep_resident(HadiSweepArgs a, int N) {
    static_assert(B == 8, "one wavefront per v-row of 8 nodes per lane");
    const int inst = hadi_xcd_remap(blockIdx.x, gridDim.x);
    if (inst >= a.n_inst) return;  // (whole block)
    const int Ni = a.ipar[inst].N < N ? a.ipar[inst].N : N;
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    if (HADI_STAMPS == 5) {
        HADI_DYN_SMEM(unsigned long long, s);
        if ((threadIdx.x & 63) < 16) s[(HADI_RES_STAMP_LDS_BYTES - 1024) / 8 + (threadIdx.x >> 6) * 16 + (threadIdx.x & 63)] = 0;
        HADI_RES_STAMP(-1);
    }
#endif
    for (int n = 1; n <= Ni; n++) {
        const bool first = n == 1;
        hadi_resident_row_phase<B>(hadi_resident_args(a), n, first);
        HADI_RES_STAMP(1);  // row loop
        hadi_resident_retire();
        hadi_resident_col_phase(hadi_resident_args(a), inst, first);
        hadi_resident_retire();
        __syncthreads();  // the next row phase's prologue fetches land in the rings Z and T alias, and read every wavefront's U rows
        HADI_RES_STAMP(6);  // final drain
    }
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    if (HADI_STAMPS == 5 && (threadIdx.x & 63) == 0) {
        HADI_DYN_SMEM(unsigned long long, s);
        for (int k = 0; k < 7; k++) atomicAdd(&g_hadi_stamps[k], s[(HADI_RES_STAMP_LDS_BYTES - 1024) / 8 + (threadIdx.x >> 6) * 16 + k]);
    }
#endif
}
