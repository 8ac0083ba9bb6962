// hadi_dispatch.h -- which kernel runs a pass: the list of instantiations, the selection, the launch geometry and the words
// of hadi_describe_last_sweep, each written once.  hadi_api.hip launches what the selectors return, hadi_create raises the
// dynamic-LDS limit over hadi_for_each_kernel, and the wave emulator (tests/emu) runs the same selectors on the host.
// No HIP runtime calls here: the header compiles under hipcc and under g++ -DHADI_EMU.  The rules: DESIGN.md section 4.1.
#pragma once
#include <stdio.h>

#include "hadi_kernels.h"
#include "hadi_plan.h"

typedef void (*HadiPassFn)(HadiSweepArgs, int);            // one pass of one time step (and the resident sweep: all steps)
typedef void (*HadiLoopFn)(HadiSweepArgs, HadiSmallArgs);  // a whole time loop in LDS

enum HadiFamily {
    HADI_F_RING, HADI_F_RING_SCH, HADI_F_STRIP, HADI_F_STRIP_SCH, HADI_F_PAIRS, HADI_F_ROW_SEQ,  // row pass
    HADI_F_COL, HADI_F_COL1, HADI_F_COL2, HADI_F_COL_SEQ,                                        // column pass
    HADI_F_RESIDENT, HADI_F_SMALL, HADI_F_SMALL_SEQ, HADI_F_SMALL_SEQ2
};
static const char *const hadi_family_name[] = {"hadi_pass_a", "hadi_pass_a_sch", "hadi_pass_a_strip", "hadi_pass_a_strip_sch",
                                               "hadi_pass_a_pairs", "hadi_pass_a_seq", "hadi_pass_b", "hadi_pass_b1", "hadi_pass_b2",
                                               "hadi_pass_b_seq", "hadi_sweep_resident", "hadi_small_kernel", "hadi_small_seq_kernel",
                                               "hadi_small_seq2_kernel"};

// One instantiation.  B: nodes per lane (column kernels: the chunk capacity MAXP); G: wavefronts per row (whole-loop kernels:
// wavefronts per instance); amer: 0 European, 1 American, 2 American in the P representation; mode: 0 Douglas step, 1 / 2
// predictor / corrector, 3 the paired strips' coupling-column table; sch: HADI_SCH_* of modes 1 / 2, else 0.
struct HadiKernel {
    int family, B, G, amer, mode, sch, f32;
    HadiPassFn fn;
    HadiLoopFn loop;  // (the whole-loop families; fn is null there)
    const char *id;   // the instantiation as the source spells it
};
#define HADI_K(fam, B, G, amer, mode, sch, f32, ...) {fam, B, G, amer, mode, sch, f32, __VA_ARGS__, nullptr, #__VA_ARGS__}
#define HADI_KL(fam, B, G, amer, ...) {fam, B, G, amer, 0, 0, 0, nullptr, __VA_ARGS__, #__VA_ARGS__}
#define HADI_K_RING_SCH(B, G, PD, SCH)                                             \
    HADI_K(HADI_F_RING_SCH, B, G, 0, 1, SCH, 0, hadi_pass_a_sch<B, G, 4, 1, PD, 1, SCH>), \
    HADI_K(HADI_F_RING_SCH, B, G, 0, 2, SCH, 0, hadi_pass_a_sch<B, G, 4, 1, PD, 2, SCH>)
#define HADI_K_RING(B, G, PD)                                                                   \
    HADI_K(HADI_F_RING, B, G, 0, 0, 0, 0, hadi_pass_a<B, G, 4, 1, PD, 0>),                      \
    HADI_K(HADI_F_RING, B, G, 1, 0, 0, 0, hadi_pass_a<B, G, 4, 1, PD, 1>),                      \
    HADI_K(HADI_F_RING, B, G, 2, 0, 0, 0, hadi_pass_a<B, G, 4, 1, PD, 2>),                      \
    HADI_K(HADI_F_RING, B, G, 0, 1, HADI_SCH_CS, 0, hadi_pass_a<B, G, 4, 1, PD, 0, 1>),         \
    HADI_K(HADI_F_RING, B, G, 0, 2, HADI_SCH_CS, 0, hadi_pass_a<B, G, 4, 1, PD, 0, 2>),         \
    HADI_K(HADI_F_RING, B, G, 0, 0, 0, 1, hadi_pass_a<B, G, 4, 1, PD, 0, 0, float>),            \
    HADI_K_RING_SCH(B, G, PD, HADI_SCH_MCS), HADI_K_RING_SCH(B, G, PD, HADI_SCH_HV)
#define HADI_K_STRIP_SCH(B, SCH)                                                       \
    HADI_K(HADI_F_STRIP_SCH, B, 1, 0, 1, SCH, 0, hadi_pass_a_strip_sch<B, 1, 1, SCH>), \
    HADI_K(HADI_F_STRIP_SCH, B, 1, 0, 2, SCH, 0, hadi_pass_a_strip_sch<B, 1, 2, SCH>)
#define HADI_K_STRIP(B)                                                                        \
    HADI_K(HADI_F_STRIP, B, 1, 0, 0, 0, 0, hadi_pass_a_strip<B, 0>),                           \
    HADI_K(HADI_F_STRIP, B, 1, 1, 0, 0, 0, hadi_pass_a_strip<B, 1>),                           \
    HADI_K(HADI_F_STRIP, B, 1, 2, 0, 0, 0, hadi_pass_a_strip<B, 2>),                           \
    HADI_K(HADI_F_STRIP, B, 1, 0, 1, HADI_SCH_CS, 0, hadi_pass_a_strip<B, 0, double, 1, 1>),   \
    HADI_K(HADI_F_STRIP, B, 1, 0, 2, HADI_SCH_CS, 0, hadi_pass_a_strip<B, 0, double, 1, 2>),   \
    HADI_K_STRIP_SCH(B, HADI_SCH_MCS), HADI_K_STRIP_SCH(B, HADI_SCH_HV)

// Every kernel the library launches through the selectors below -- they return entries of this table and nothing else.
// (Internal linkage, here and for everything that reaches the table: the static local of an inline function is ONE object
// for all the shared libraries of a process, and the emulator's test libraries would hand each other their kernels.)
static inline const HadiKernel *hadi_kernel_table(int *count) {
    static const HadiKernel tab[] = {
        HADI_K_RING(1, 1, 2), HADI_K_RING(2, 1, 2), HADI_K_RING(4, 1, 2), HADI_K_RING(8, 1, 1), HADI_K_RING(8, 2, 1),
        HADI_K_STRIP(2), HADI_K_STRIP(4), HADI_K_STRIP(8),
        HADI_K(HADI_F_STRIP, 8, 1, 0, 0, 0, 1, hadi_pass_a_strip<8, 0, float>),
        HADI_K(HADI_F_STRIP, 8, 2, 0, 0, 0, 1, hadi_pass_a_strip<8, 0, float, 2>),
        HADI_K(HADI_F_STRIP, 8, 2, 0, 0, 0, 0, hadi_pass_a_strip<8, 0, double, 2>),
        HADI_K(HADI_F_STRIP, 8, 2, 1, 0, 0, 0, hadi_pass_a_strip<8, 1, double, 2>),
        HADI_K(HADI_F_STRIP, 8, 2, 2, 0, 0, 0, hadi_pass_a_strip<8, 2, double, 2>),
        HADI_K(HADI_F_STRIP, 8, 2, 0, 1, HADI_SCH_CS, 0, hadi_pass_a_strip<8, 0, double, 2, 1>),
        HADI_K(HADI_F_STRIP, 8, 2, 0, 2, HADI_SCH_CS, 0, hadi_pass_a_strip<8, 0, double, 2, 2>),
        HADI_K(HADI_F_STRIP, 8, 2, 0, 3, 0, 0, hadi_pass_a_strip<8, 0, double, 2, 3>),  // (hadi_select_pair_table)
        HADI_K(HADI_F_STRIP_SCH, 8, 2, 0, 2, HADI_SCH_MCS, 0, hadi_pass_a_strip_sch<8, 2, 2, HADI_SCH_MCS>),
        HADI_K(HADI_F_STRIP_SCH, 8, 2, 0, 2, HADI_SCH_HV, 0, hadi_pass_a_strip_sch<8, 2, 2, HADI_SCH_HV>),
        HADI_K(HADI_F_PAIRS, 4, 1, 0, 0, 0, 0, hadi_pass_a_pairs<0>),
        HADI_K(HADI_F_PAIRS, 4, 1, 1, 0, 0, 0, hadi_pass_a_pairs<1>),
        HADI_K(HADI_F_PAIRS, 4, 1, 2, 0, 0, 0, hadi_pass_a_pairs<2>),
        HADI_K(HADI_F_ROW_SEQ, 0, 0, 0, 0, 0, 0, hadi_pass_a_seq<0>),
        HADI_K(HADI_F_ROW_SEQ, 0, 0, 1, 0, 0, 0, hadi_pass_a_seq<1>),
        HADI_K(HADI_F_COL, 8, 0, 0, 0, 0, 0, hadi_pass_b<8, 0>),
        HADI_K(HADI_F_COL, 8, 0, 1, 0, 0, 0, hadi_pass_b<8, 1>),
        HADI_K(HADI_F_COL, 8, 0, 2, 0, 0, 0, hadi_pass_b<8, 2>),
        HADI_K(HADI_F_COL, 8, 0, 0, 0, 0, 1, hadi_pass_b<8, 0, float>),
        HADI_K(HADI_F_COL1, 16, 0, 0, 0, 0, 0, hadi_pass_b1<16, 0>),
        HADI_K(HADI_F_COL1, 16, 0, 1, 0, 0, 0, hadi_pass_b1<16, 1>),
        HADI_K(HADI_F_COL1, 16, 0, 2, 0, 0, 0, hadi_pass_b1<16, 2>),
        HADI_K(HADI_F_COL1, 16, 0, 0, 0, 0, 1, hadi_pass_b1<16, 0, float>),
        HADI_K(HADI_F_COL2, 16, 0, 0, 0, 0, 0, hadi_pass_b2<16, double, HADI_B2_NPF(8)>),
        HADI_K(HADI_F_COL2, 16, 0, 0, 0, 0, 1, hadi_pass_b2<16, float, HADI_B2_NPF(4)>),
        HADI_K(HADI_F_COL_SEQ, 0, 0, 0, 0, 0, 0, hadi_pass_b_seq<0>),
        HADI_K(HADI_F_COL_SEQ, 0, 0, 1, 0, 0, 0, hadi_pass_b_seq<1>),
        HADI_K(HADI_F_RESIDENT, 8, 1, 0, 0, 0, 0, hadi_sweep_resident<8>),  // (hadi_select_resident)
        HADI_KL(HADI_F_SMALL, 1, 4, 0, hadi_small_kernel<1, 4, false>), HADI_KL(HADI_F_SMALL, 1, 4, 1, hadi_small_kernel<1, 4, true>),
        HADI_KL(HADI_F_SMALL, 2, 4, 0, hadi_small_kernel<2, 4, false>), HADI_KL(HADI_F_SMALL, 2, 4, 1, hadi_small_kernel<2, 4, true>),
        HADI_KL(HADI_F_SMALL, 1, 8, 0, hadi_small_kernel<1, 8, false>), HADI_KL(HADI_F_SMALL, 1, 8, 1, hadi_small_kernel<1, 8, true>),
        HADI_KL(HADI_F_SMALL, 2, 8, 0, hadi_small_kernel<2, 8, false>), HADI_KL(HADI_F_SMALL, 2, 8, 1, hadi_small_kernel<2, 8, true>),
        HADI_KL(HADI_F_SMALL_SEQ, 1, 1, 0, hadi_small_seq_kernel<1>), HADI_KL(HADI_F_SMALL_SEQ, 2, 1, 0, hadi_small_seq_kernel<2>),
        HADI_KL(HADI_F_SMALL_SEQ2, 1, 1, 0, hadi_small_seq2_kernel<1>), HADI_KL(HADI_F_SMALL_SEQ2, 2, 1, 0, hadi_small_seq2_kernel<2>),
    };
    *count = (int)(sizeof(tab) / sizeof(tab[0]));
    return tab;
}
#undef HADI_K
#undef HADI_KL
#undef HADI_K_RING_SCH
#undef HADI_K_RING
#undef HADI_K_STRIP_SCH
#undef HADI_K_STRIP

// The LDS-resident whole-loop kernels of the predictor-corrector schemes (hadi_k_small_sch.h), launched from run_sweep
// outside the table as the team and Greeks kernels are.  B: 1 or 2 nodes per lane of the packed layout; sch: HADI_SCH_*.
// Null where no such instantiation exists: an error for the caller, never a fallback.
static inline HadiLoopFn hadi_small_sch_fn(int B, int sch) {
    if (B == 1) return sch == HADI_SCH_CS ? hadi_small_sch_kernel<1, HADI_SCH_CS> : sch == HADI_SCH_MCS ? hadi_small_sch_kernel<1, HADI_SCH_MCS> :
                       sch == HADI_SCH_HV ? hadi_small_sch_kernel<1, HADI_SCH_HV> : (HadiLoopFn) nullptr;
    if (B == 2) return sch == HADI_SCH_CS ? hadi_small_sch_kernel<2, HADI_SCH_CS> : sch == HADI_SCH_MCS ? hadi_small_sch_kernel<2, HADI_SCH_MCS> :
                       sch == HADI_SCH_HV ? hadi_small_sch_kernel<2, HADI_SCH_HV> : (HadiLoopFn) nullptr;
    return nullptr;
}
// Its admission (the grid alone: what run_sweep adds is the call's) and its dynamic LDS bytes: m1 <= 128, m2 <= 32 and the
// kernel's own layout within the CU's 160 KiB.
static inline size_t hadi_small_sch_smem(const HadiLayout &L) { return (size_t)hadi_small_sch_layout(L.m1, L.nrows).total * sizeof(double); }
static inline bool hadi_small_sch_admits(const HadiLayout &L) {
    return L.G == 1 && L.B <= 2 && L.P == 1 && hadi_small_sch_smem(L) <= (size_t)160 * 1024;
}

// The whole-loop LDS kernel of a sampled Bates ladder (hadi_small_jump_kernel, hadi_k_small.h): hadi_small_kernel<B, W, false> with the
// jump sub-step inside the time loop, launched from run_sweep outside the table as hadi_small_sch_kernel is.  B: 1 or 2 nodes per
// lane; W: 4 or 8 wavefronts per instance.  Null where no such instantiation exists: an error for the caller, never a fallback.
static inline HadiLoopFn hadi_small_jump_fn(int B, int W) {
    if (B == 1) return W == 4 ? hadi_small_jump_kernel<1, 4> : W == 8 ? hadi_small_jump_kernel<1, 8> : (HadiLoopFn) nullptr;
    if (B == 2) return W == 4 ? hadi_small_jump_kernel<2, 4> : W == 8 ? hadi_small_jump_kernel<2, 8> : (HadiLoopFn) nullptr;
    return nullptr;
}

// Calls f with the address of every kernel of the table, of the two instance-resident team kernels (their own argument
// block), of the predictor-corrector schemes' LDS-resident kernels (hadi_small_sch_fn) and of the sampled Bates ladder's
// (hadi_small_jump_fn).  hadi_create raises the
// dynamic-LDS limit of each: no kernel that needs more than the default can be left out.
template <class F>
static void hadi_for_each_kernel(F f) {
    int n;
    const HadiKernel *t = hadi_kernel_table(&n);
    for (int i = 0; i < n; i++) {
        if (t[i].fn) f(t[i].fn);
        else f(t[i].loop);
    }
    f(hadi_team_kernel<8>);
    f(hadi_team_kernel<4>);
    for (int B = 1; B <= 2; B++)
        for (int sch = HADI_SCH_CS; sch <= HADI_SCH_HV; sch++) f(hadi_small_sch_fn(B, sch));
    for (int B = 1; B <= 2; B++)
        for (int W = 4; W <= 8; W += 4) f(hadi_small_jump_fn(B, W));
}

// A selected kernel and its launch geometry.  k is null when the table holds no such instantiation: an error, never a fallback.
struct HadiSel {
    const HadiKernel *k;
    unsigned grid, block;
    size_t smem;  // dynamic LDS bytes
};
static inline HadiSel hadi_sel(int family, int B, int G, int amer, int mode, int sch, int f32, long long grid, int block, size_t smem) {
    int n;
    const HadiKernel *t = hadi_kernel_table(&n);
    for (int i = 0; i < n; i++)
        if (t[i].family == family && t[i].B == B && t[i].G == G && t[i].amer == amer && t[i].mode == mode && t[i].sch == sch && t[i].f32 == f32)
            return HadiSel{t + i, (unsigned)grid, (unsigned)block, smem};
    return HadiSel{nullptr, 0, 0, 0};
}

// Everything the choice of a pass kernel depends on.  scheme: enum hadi_scheme (0 Douglas, 1 Craig-Sneyd, 2 MCS, 3 HV).
struct HadiPassCtx {
    const HadiPlan &pl;              // launch geometry of THIS sub-batch
    int n_inst;                      // its instances
    bool american, amp, xstep, f32;  // amp: P representation; xstep: this step runs on the explicit (U, lambda_bar) pair
    int scheme;                      // which predictor / corrector kernels modes 1 / 2 run
    int cs_strips;                   // predictor-corrector row passes on strips where the plan chose strips: 0 never, 1 both,
                                     // 2 / 3 (diagnostics) only the predictor / only the corrector
    int col_prefetch;                // hadi_pass_b2 for European sweeps of 9 .. 16 chunks
};

// Row pass of one time step.  mode: 0 Douglas, 1 / 2 predictor / corrector of c.scheme.
static inline HadiSel hadi_select_row_pass(const HadiPassCtx &c, int mode) {
    const HadiPlan &pl = c.pl;
    const HadiLayout &L = pl.L;
    const int sch = !mode ? 0 : c.scheme == 2 ? HADI_SCH_MCS : c.scheme == 3 ? HADI_SCH_HV : HADI_SCH_CS;
    const int nt_ring = 64 * pl.W * L.G * pl.NG, nt_strip = 64 * HADI_STRIP_WAVES(L.B);
    const bool sch_own = sch == HADI_SCH_MCS || sch == HADI_SCH_HV;  // the scheme's own kernels (hadi_pass_a_sch / _strip_sch)
    const bool cs_on_strips = pl.use_strip && mode != 0 && !pl.use_pairs && (c.cs_strips == 1 || c.cs_strips == 1 + mode);
    if (sch_own) {
        // (paired strips: the corrector only -- the predictor of those shapes runs on the shared ring, see hadi_pass_a_strip_sch)
        if (cs_on_strips && !(L.G == 2 && mode == 1)) return hadi_sel(HADI_F_STRIP_SCH, L.B, L.G, 0, mode, sch, 0, pl.grid_as, nt_strip, pl.smem_as);
        return hadi_sel(HADI_F_RING_SCH, L.B, L.G, 0, mode, sch, 0, pl.grid_a, nt_ring, pl.smem_a);
    }
    const size_t payoff_row = (size_t)L.rowp * sizeof(double);  // P representation: the payoff row behind the tables in LDS
    if (pl.row_seq)  // more than 1024 s-intervals: one lane per v-row, sequential along s
        return hadi_sel(HADI_F_ROW_SEQ, 0, 0, c.american ? 1 : 0, 0, 0, 0, (long long)c.n_inst * ((L.nrows + 63) / 64), 64, 0);
    if (pl.use_pairs && pl.use_strip && mode == 0 && !c.f32) {  // 4 nodes per lane: two strips per wavefront
        const int amer = (c.amp && !c.xstep) ? 2 : c.american ? 1 : 0;
        return hadi_sel(HADI_F_PAIRS, 4, 1, amer, 0, 0, 0, pl.grid_as, 64 * HADI_PAIR_WAVES, amer == 2 ? pl.smem_pairs_amp : pl.smem_pairs_eu);
    }
    if (c.amp && !c.xstep) {  // P representation: barrier-free strips (one or two wavefronts per row) or the shared ring
        if (pl.use_strip && mode == 0) return hadi_sel(HADI_F_STRIP, L.B, L.G, 2, 0, 0, 0, pl.grid_as, nt_strip, pl.smem_as + payoff_row);
        return hadi_sel(HADI_F_RING, L.B, L.G, 2, 0, 0, 0, pl.grid_a, nt_ring, pl.smem_a + payoff_row);
    }
    if (c.f32) {  // fp32 state: the rings hold floats (the coefficient arrays and tables stay double)
        if (pl.use_strip && L.B == 8 && L.G == 2) return hadi_sel(HADI_F_STRIP, 8, 2, 0, 0, 0, 1, pl.grid_as, nt_strip, pl.smem_as);
        if (pl.use_strip && L.B == 8)
            return hadi_sel(HADI_F_STRIP, 8, 1, 0, 0, 0, 1, pl.grid_as, nt_strip, (size_t)8 * 4 * L.rowp * sizeof(float) + (size_t)4 * 64 * L.B * sizeof(double));
        const size_t ring_elems = (size_t)pl.NG * ((pl.PD + 1) * pl.W + 4) * L.rowp;
        return hadi_sel(HADI_F_RING, L.B, L.G, 0, 0, 0, 1, pl.grid_a, nt_ring, pl.smem_a - ring_elems * (sizeof(double) - sizeof(float)));
    }
    if (cs_on_strips) return hadi_sel(HADI_F_STRIP, L.B, L.G, 0, mode, sch, 0, pl.grid_as, nt_strip, pl.smem_as);  // Craig-Sneyd (European, fp64)
    if (pl.use_strip && mode == 0) return hadi_sel(HADI_F_STRIP, L.B, L.G, c.american ? 1 : 0, 0, 0, 0, pl.grid_as, nt_strip, pl.smem_as);
    return hadi_sel(HADI_F_RING, L.B, L.G, (mode == 0 && c.american) ? 1 : 0, mode, sch, 0, pl.grid_a, nt_ring, pl.smem_a);
}

// Column pass of one time step.  Up to 8 chunks: 512-thread blocks with two register buffers (2 waves per SIMD); 9 .. 16
// chunks: the 1024-thread block leaves 128 VGPRs per lane, which only the single-buffer kernels fit (measured at 1024x512:
// 0.250 vs 0.382 ms/launch for the double-buffered code, which spills).
static inline HadiSel hadi_select_col_pass(const HadiPassCtx &c) {
    const HadiPlan &pl = c.pl;
    if (pl.col_seq)  // more than 16 chunks of v-rows: one lane per storage column, sequential along v
        return hadi_sel(HADI_F_COL_SEQ, 0, 0, c.american ? 1 : 0, 0, 0, 0, (long long)c.n_inst * pl.ctiles, 64, 0);
    const int amer = (c.amp && !c.xstep) ? 2 : (c.american && !c.f32) ? 1 : 0, f32 = (amer != 2 && c.f32) ? 1 : 0;
    if (pl.L.P <= 8) return hadi_sel(HADI_F_COL, 8, 0, amer, 0, 0, f32, pl.grid_b, pl.block_b, pl.smem_b);
    if (amer == 0 && c.col_prefetch) return hadi_sel(HADI_F_COL2, 16, 0, 0, 0, 0, f32, pl.grid_b, pl.block_b, pl.smem_b2);
    return hadi_sel(HADI_F_COL1, 16, 0, amer, 0, 0, f32, pl.grid_b, pl.block_b, pl.smem_b);
}

// The whole-loop kernels of small grids.  kind (decided by the caller, it depends on the handle): 0 a block per instance with
// `waves` (4 or 8) wavefronts, 1 one wavefront per instance with sequential line solves, 2 two instances per wavefront.
static inline size_t hadi_small_seq_smem(const HadiLayout &L) { return (size_t)hadi_small_seq_layout(L.m1, L.nrows).total * sizeof(double); }
static inline HadiSel hadi_select_small(const HadiPlan &pl, int n_inst, int kind, int waves, bool american) {
    const int B = pl.L.B == 1 ? 1 : 2;
    if (kind == 2) return hadi_sel(HADI_F_SMALL_SEQ2, B, 1, 0, 0, 0, 0, (n_inst + 1) / 2, 64, 2 * hadi_small_seq_smem(pl.L));
    if (kind == 1) return hadi_sel(HADI_F_SMALL_SEQ, B, 1, 0, 0, 0, 0, n_inst, 64, hadi_small_seq_smem(pl.L));
    const int W = waves == 8 ? 8 : 4;
    return hadi_sel(HADI_F_SMALL, B, W, american ? 1 : 0, 0, 0, 0, n_inst, 64 * W, american ? pl.smem_small_am : pl.smem_small_eu);
}
// Paired strips (Douglas steps): the pairs' coupling column, built once per solve.  Its own LDS size: the fp64 ring of 4 pairs
// x 3 slots, whatever the state precision of the sweep.
static inline HadiSel hadi_select_pair_table(const HadiPlan &pl) {
    return hadi_sel(HADI_F_STRIP, 8, 2, 0, 3, 0, 0, pl.grid_as, 512,
                    (size_t)4 * HADI_STRIP_NS(8, 2, 8) * pl.L.rowp * sizeof(double) + ((size_t)4 * 64 * 8 * 2 + (size_t)4 * 16) * sizeof(double));
}
// Resident sweep: one block per instance (LDS: the strip rings and coefficient arrays, RT behind them; the column phase's
// exchange values and product alias the rings).
static inline HadiSel hadi_select_resident(const HadiPlan &pl) {
    size_t smem = hadi_resident_smem(pl.L);  // (above the column pass's own smem_b: that layout fits the first three rings)
#if defined(HADI_STAMPS) && HADI_STAMPS == 5
    smem = 163840;  // (diagnostic build: the stamps' sums live in the last KiB)
#endif
    return hadi_sel(HADI_F_RESIDENT, 8, 1, 0, 0, 0, 0, pl.grid_as, 64 * HADI_STRIP_WAVES(8), smem);
}
// Instance-resident launch (hadi_team_kernel<8 | 4>): dynamic LDS bytes.
static inline size_t hadi_team_smem(const HadiLayout &L, bool have_div) {
    return ((size_t)4 * 64 * L.B + hadi_pb_mf_doubles(L.P) + (size_t)L.P * HADI_LC * HADI_PBW + (have_div ? (size_t)(L.m1 + 2) + (size_t)8 * L.rowp : 0)) * sizeof(double) + 64;
}

// ---- the selection in words ------------------------------------------------------------------------------------------------
// The kernel as hadi_describe_last_sweep spells it (template values of the plan where the source has them).
static inline int hadi_kernel_name(const HadiKernel &k, const HadiPlan &pl, char *out, size_t cap) {
    const char *fam = hadi_family_name[k.family], *tag = k.amer == 2 ? "AM-P" : k.amer == 1 ? "AM" : "EU";
    const char *sch = k.sch == HADI_SCH_MCS ? "MCS" : k.sch == HADI_SCH_HV ? "HV" : "CS";
    const bool cs = k.mode == 1 || k.mode == 2;
    switch (k.family) {
        case HADI_F_RING: case HADI_F_RING_SCH:
            return snprintf(out, cap, "%s<%d,%d,%d,%d,%d,%s%s%s%s>", fam, k.B, k.G, pl.W, pl.NG, pl.PD, tag, k.f32 ? ",float" : "", cs ? "," : "", cs ? sch : "");
        case HADI_F_STRIP: case HADI_F_STRIP_SCH:
            if (cs) return snprintf(out, cap, "%s<%d,EU,double,%d,%s>", fam, k.B, k.G, sch);
            if (k.G == 2) return snprintf(out, cap, "%s<%d,%s,%s,2>", fam, k.B, tag, k.f32 ? "float" : "double");
            return snprintf(out, cap, "%s<%d,%s%s>", fam, k.B, tag, k.f32 ? ",float" : "");
        case HADI_F_COL: case HADI_F_COL1: case HADI_F_COL2: return snprintf(out, cap, "%s<%d,%s>", fam, k.B, tag);
        default: return snprintf(out, cap, "%s<%s>", fam, tag);  // pairs and the sequential passes
    }
}
// "row pass ... ; column pass ..." of a sub-batch, from what the selectors return for it: the Douglas step, or the corrector
// of a predictor-corrector scheme.  `cs_strips` 2 / 3 (diagnostics) are worded as 1: the text names the strip kernel where one
// of the two row passes runs on the shared ring.
static inline int hadi_describe_passes(HadiPassCtx c, char *out, size_t cap) {
    const HadiPlan &pl = c.pl;
    c.xstep = false;
    c.cs_strips = c.cs_strips ? 1 : 0;
    const HadiSel row = hadi_select_row_pass(c, c.scheme ? 2 : 0), col = hadi_select_col_pass(c);
    if (!row.k || !col.k) return snprintf(out, cap, "no kernel for this shape");
    const char *extra = row.k->amer == 2 ? ", no lambda_bar array" : row.k->f32 ? ", fp32 state" : "";
    char rown[96], coln[64], what[128];
    hadi_kernel_name(*row.k, pl, rown, sizeof rown);
    hadi_kernel_name(*col.k, pl, coln, sizeof coln);
    switch (row.k->family) {
        case HADI_F_RING: case HADI_F_RING_SCH: snprintf(what, sizeof what, "tiles of %d rows%s", pl.R, extra); break;
        case HADI_F_STRIP: case HADI_F_STRIP_SCH:
            snprintf(what, sizeof what, "%sstrips of %d rows%s%s", row.k->G == 2 ? "paired " : "", pl.RS, extra,
                     row.k->family == HADI_F_STRIP_SCH && row.k->G == 2 ? "; the predictor on hadi_pass_a_sch" : "");
            break;
        case HADI_F_PAIRS: snprintf(what, sizeof what, "two strips of %d rows per wavefront%s", pl.RS, extra); break;
        default: snprintf(what, sizeof what, "one lane per v-row, sequential along s"); break;
    }
    if (col.k->family == HADI_F_COL_SEQ)
        return snprintf(out, cap, "row pass %s (%s); column pass %s (one lane per column, sequential along v)", rown, what, coln);
    return snprintf(out, cap, "row pass %s (%s); column pass %s (%d chunks of %d rows, %d column tiles per block)", rown, what, coln,
                    pl.L.P, HADI_LC, pl.btpw);
}
