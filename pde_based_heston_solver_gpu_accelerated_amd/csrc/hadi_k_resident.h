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
// LDS: [8 rings of 4 rows][4 s-coefficient arrays] as in hadi_pass_a_strip; the column phase's exchange values, selected
// inverse rows and their product (hadi_pb_mf_doubles) alias the rings.

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

// Row phase: hadi_pass_a_strip<B, 0, double, 1, 0> for step n.
template <int B>
HADI_DEV HADI_FORCEINLINE void hadi_resident_row_phase(const HadiSweepArgs &a, int n) {
    HADI_RESIDENT_TID
    constexpr int AMER = 0, G = 1, MODE = 0, SCH = HADI_SCH_CS;
    typedef double T;
#include "hadi_k_row_strip_body.h"
}

// Column phase: the European branch of hadi_pass_b<8, 0, double> with ONE block per instance -- all ctiles tiles, the short
// one last.  Wavefronts without a chunk (P < 8) only take part in the block barriers of every tile's reduced system.
HADI_DEV HADI_FORCEINLINE void hadi_resident_col_phase(const HadiSweepArgs &a, int inst) {
    HADI_DYN_SMEM(double, smem);
    HADI_RESIDENT_TID
    HadiPassBCtx c;
    c.lane = threadIdx.x & 63;
    c.wave = HADI_UNIFORM((int)(threadIdx.x >> 6));
    c.P = a.L.P;
    const int P = c.P, cnt = a.ctiles;
    if (c.wave >= P) {
        __syncthreads();  // (the column LDS is set up)
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
    HadiTileSet ts;  // (hadi_pb_tiles of one block per instance: the full tiles in order, then the short one)
    ts.first = 0; ts.stride = 1; ts.nfull_mine = a.L.rowp >> 6; ts.short_tile = ts.nfull_mine; ts.cnt = cnt;
    auto tile = [&](int i) { return hadi_pb_tile(ts, i); };
#if defined(HADI_STAMPS) && !defined(HADI_EMU)
    unsigned long long stamp_store_[32] = {0};
    c.stamp_acc_ = stamp_store_;
#endif
    double ya[HADI_LC], yb[HADI_LC], yc[HADI_LC];
    hadi_pb_load<double>(c, tile(0), ya);
    hadi_pb_load_table(c, a.pb + ((size_t)inst * a.L.nrows_pad + c.ja) * HADI_PBW);
    hadi_pb_setup_lds<HADI_PB_MF != 0>(c, smem, a.rinv + (size_t)inst * 16 * P * P, 2);
    c.inv_dt = 1.0 / ip.dt;
    c.dt = ip.dt;
    __syncthreads();
    if (1 < cnt) hadi_pb_load<double>(c, tile(1), yb);
    for (int i = 0; i < cnt; i += 3) {
        if (i + 2 < cnt) hadi_pb_load<double>(c, tile(i + 2), yc);
        hadi_pb_solve_store<0, double>(c, tile(i), i & 1, ya, 0);
        if (i + 1 < cnt) {
            if (i + 3 < cnt) hadi_pb_load<double>(c, tile(i + 3), ya);
            hadi_pb_solve_store<0, double>(c, tile(i + 1), (i + 1) & 1, yb, 0);
        }
        if (i + 2 < cnt) {
            if (i + 4 < cnt) hadi_pb_load<double>(c, tile(i + 4), yb);
            hadi_pb_solve_store<0, double>(c, tile(i + 2), (i + 2) & 1, yc, 0);
        }
    }
}

// Every wavefront's loads and stores have retired (its Y / U rows are in the CU's L1 and L2), then the block meets.
HADI_DEV HADI_FORCEINLINE void hadi_resident_drain() {
#if !defined(HADI_EMU)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}

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

// Grid: the sub-batch's instances, padded to a multiple of 8 (the strip body's XCD remap: logical block = instance).
// N: the sweep's step count; an instance with fewer steps (per-instance maturities) stops at its own.
// `a` MUST stay the first parameter: hadi_resident_args() reads the argument block at offset 0 of the kernarg segment
// (tests/test_isa_resident.py checks that the kernel's metadata puts it there).
template <int B>
__global__ void __launch_bounds__(64 * HADI_STRIP_WAVES(B), 2) hadi_sweep_resident(HadiSweepArgs a, int N) {
    static_assert(B == 8, "one wavefront per v-row of 8 nodes per lane");
    const int inst = hadi_xcd_remap(blockIdx.x, gridDim.x);
    if (inst >= a.n_inst) return;  // (whole block)
    const int Ni = a.ipar[inst].N < N ? a.ipar[inst].N : N;
    for (int n = 1; n <= Ni; n++) {
        hadi_resident_row_phase<B>(hadi_resident_args(a), n);
        hadi_resident_drain();
        hadi_resident_col_phase(hadi_resident_args(a), inst);
        hadi_resident_drain();
    }
}
