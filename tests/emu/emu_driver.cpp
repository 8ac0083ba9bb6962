// emu_driver.cpp -- TEST-ONLY.  Runs csrc/hadi_kernels.h (the product's kernel source, unmodified)
// under the host-thread wave emulator so tests can compare its logic with the oracle without a GPU.
// Never shipped, never linked into libhadi; see wave_emu.h.
#define HADI_EMU 1
#include "hadi_route.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace emu {
thread_local emu_dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockState *t_block;
thread_local WaveState *t_wave;
thread_local int t_lane;
}  // namespace emu

// kernel-selection overrides, the emulator's stand-in for hadi_set_tuning
static HadiTuning g_tune;
static int g_err = 0, g_debug = 0;  // the handle's device error word and the "debug_fault" test hook
static int g_tile_il = 0;           // "tile_interleave": the column pass's blocks take their full tiles interleaved (opt-in, as in the library)
static int g_cs_strips = 1;         // "cs_strips": predictor-corrector row passes on strips where the plan chose strips (default, as in
                                    // the library); 2 / 3: only the predictor / only the corrector on strips, the other on the ring
static int g_team_blocks = 1;       // "team_blocks": blocks per team of the instance-resident launch (> 1: the grid's blocks run concurrently)
static int g_col_prefetch = 0;      // "col_prefetch": hadi_pass_b2 for European sweeps of 9 .. 16 chunks (opt-in, as in the library)
extern "C" int emu_take_error() { const int e = g_err; g_err = 0; return e; }
extern "C" int emu_set_tuning(const char *key, int value) {
    const std::string k(key);
    if (k == "debug_fault") g_debug = value;
    else if (k == "strip") g_tune.strip = value < 0 ? -1 : (value ? 1 : 0);
    else if (k == "row_tile") g_tune.row_tile = value > 0 ? value : 0;
    else if (k == "strip_blocks") g_tune.strip_blocks = value > 0 ? value : 0;
    else if (k == "pair_strips") g_tune.pair_strips = value < 0 ? -1 : (value ? 1 : 0);
    else if (k == "col_groups") g_tune.col_groups = value > 0 ? value : 0;
    else if (k == "col_prefetch") g_col_prefetch = value ? 1 : 0;
    else if (k == "cs_strips") g_cs_strips = (value >= 0 && value <= 3) ? value : 1;  // (as hadi_set_tuning)
    else if (k == "team_blocks") g_team_blocks = value > 0 ? value : 1;
    else if (k == "tile_interleave") g_tile_il = value ? 1 : 0;
    else if (k == "reset") { g_tune = HadiTuning(); g_debug = 0; g_col_prefetch = 0; g_tile_il = 0; g_cs_strips = 1; g_team_blocks = 1; }
    else return 1;
    return 0;
}

// The library's own dispatch (csrc/hadi_dispatch.h): select as hadi_api.hip does, then run the kernel on the emulator.
// Returns 2 where the table holds no kernel for the pass.
static int run_pass(const HadiSel &sel, const HadiSweepArgs &a, int n) {
    if (!sel.k) return 2;
    emu::launch(sel.grid, sel.block, [&]() { sel.k->fn(a, n); }, sel.smem);
    return 0;
}

// The selection alone, for tests/test_kernel_selection.py.  in[16]: m1, m2, instances, target_waves, "strip", "pair_strips",
// no_strips (the caller's theta = 0 or r_d = r_f: run_sweep clears use_strip), american, amp, xstep, f32, scheme (enum
// hadi_scheme), "cs_strips", "col_prefetch", mode, what (0 the row pass, 1 the column pass, 2 entry in[0] of the table of
// instantiations whatever the other inputs).  o[11]: table index, family, B, G, amer, mode, sch, f32, grid, block, LDS
// bytes; name: the kernel as the description spells it (what = 2: as the source spells it); desc: the description of the
// sub-batch.  Returns 0, 1 (no plan), 2 (no kernel); what = 2: the number of table entries.
extern "C" int emu_select(const int *in, long long *o, char *name, char *desc, int cap) {
    int count;
    const HadiKernel *tab = hadi_kernel_table(&count);
    auto put = [&](const HadiKernel *k) {
        const long long v[8] = {k - tab, k->family, k->B, k->G, k->amer, k->mode, k->sch, k->f32};
        std::copy(v, v + 8, o);
    };
    if (in[15] == 2) {
        if (in[0] < 0 || in[0] >= count) return count;
        put(tab + in[0]);
        std::snprintf(name, cap, "%s", tab[in[0]].id);
        return count;
    }
    HadiTuning tu;
    tu.strip = in[4]; tu.pair_strips = in[5];
    HadiPlan pl;
    if (hadi_make_plan(in[0], in[1], in[2], in[3], &pl, tu, in[10] ? 4 : 8)) return 1;
    if (in[6]) pl.use_strip = 0;
    const HadiPassCtx pc{pl, in[2], in[7] != 0, in[8] != 0, in[9] != 0, in[10] != 0, in[11], in[12], in[13]};
    const HadiSel sel = in[15] ? hadi_select_col_pass(pc) : hadi_select_row_pass(pc, in[14]);
    if (!sel.k) return 2;
    put(sel.k);
    o[8] = sel.grid; o[9] = sel.block; o[10] = (long long)sel.smem;
    hadi_kernel_name(*sel.k, pl, name, cap);
    hadi_describe_passes(pc, desc, cap);
    return 0;
}

// The route of a whole call (csrc/hadi_route.h: what run_sweep consumes), for tests/test_route_selection.py.  in[16]: CUs,
// instances, m1, m2, variant, scheme, state precision (enums of hadi.h), r_d == r_f, debug, profiling, n_snap, dividends,
// uniform_steps, team_failed, amp (the caller's payoff-shape read-back), what became of a team launch (HADI_TEAM_*); tuning:
// "key=value,..." through the table hadi_set_tuning walks.  o[15]: status, kind, small_waves, sub-batches, two_streams,
// fork_before, resident sub-batches, read_payoff_shape, pair_tab, need_lam_u0, need_ut, need_f32, need_v_r1_c2, need_r1,
// graphable; subs: off, cnt, lane, resident of the first max_subs sub-batches; desc: hadi_describe_last_sweep's text.
// Returns 0, 1 (no route: o[0] says why) or 2 (a tuning key or value the table refuses).
extern "C" int emu_route(const int *in, double theta, const char *tuning, long long *o, int *subs, int max_subs, char *desc, int cap) {
    HadiRouteIn ri;
    ri.cu_count = in[0]; ri.n = in[1]; ri.m1 = in[2]; ri.m2 = in[3]; ri.variant = in[4]; ri.scheme = in[5]; ri.prec = in[6];
    ri.theta = theta; ri.rates_equal = in[7] != 0; ri.debug = in[8]; ri.profiling = in[9] != 0; ri.n_snap = in[10];
    ri.dividends = in[11] != 0; ri.uniform_steps = in[12] != 0; ri.team_failed = in[13] != 0;
    for (std::string rest(tuning ? tuning : ""); !rest.empty();) {
        const size_t comma = rest.find(','), eq = rest.find('=');
        if (eq == std::string::npos || eq > comma) return 2;
        const HadiTuneKey *e = hadi_tuning_key(rest.substr(0, eq).c_str());
        if (!e || hadi_tuning_set(ri.t, *e, std::atoi(rest.c_str() + eq + 1))) return 2;
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
    }
    const HadiRoute r = hadi_route(ri);
    o[0] = r.status;
    if (r.status) return 1;
    const long long v[15] = {r.status, r.kind, r.small_waves, (long long)r.bp.subs.size(), r.bp.two_streams, r.bp.fork_before, r.n_resident(),
                             r.read_payoff_shape, r.pair_tab, r.need_lam_u0, r.need_ut, r.need_f32, r.need_v_r1_c2, r.need_r1, r.graphable};
    std::copy(v, v + 15, o);
    for (int k = 0; k < (int)r.bp.subs.size() && k < max_subs; k++) {
        const int s4[4] = {r.bp.subs[k].off, r.bp.subs[k].cnt, r.bp.subs[k].lane, r.resident[k]};
        std::copy(s4, s4 + 4, subs + 4 * k);
    }
    std::snprintf(desc, cap, "%s", hadi_describe_route(r, ri, in[14] != 0, in[15]).c_str());
    return 0;
}

extern "C" int emu_plan(int m1, int m2, int n_inst, int target_waves, int *out /*B,rowp,P,R,ntiles,ctiles*/) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, target_waves, &pl, g_tune)) return 1;
    out[0] = pl.L.B; out[1] = pl.L.rowp; out[2] = pl.L.P; out[3] = pl.R; out[4] = pl.ntiles; out[5] = pl.L.G;
    return 0;
}

// every launch-geometry field of the plan, for the host-logic invariants test
extern "C" int emu_plan_full(int m1, int m2, int n_inst, int target_waves, long long *o /*[26]*/) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, target_waves, &pl, g_tune)) return 1;
    const HadiLayout &L = pl.L;
    o[0] = L.B; o[1] = L.G; o[2] = L.rowp; o[3] = L.P; o[4] = L.nrows; o[5] = L.nrows_pad; o[6] = L.inst_stride;
    o[7] = pl.W; o[8] = pl.NG; o[9] = pl.PD; o[10] = pl.R; o[11] = pl.ntiles; o[12] = pl.grid_a; o[13] = (long long)pl.smem_a;
    o[14] = pl.use_strip; o[15] = pl.RS; o[16] = pl.sblocks; o[17] = pl.grid_as; o[18] = (long long)pl.smem_as;
    o[19] = pl.ctiles; o[20] = pl.btpw; o[21] = pl.bgroups; o[22] = pl.grid_b; o[23] = (long long)pl.smem_b;
    o[24] = pl.use_pairs; o[25] = (long long)pl.smem_pairs_amp;
    return 0;
}

// the column tiles block `grp` of an instance walks, in order (hadi_pb_tiles); returns their number
extern "C" int emu_col_tiles(int m1, int m2, int n_inst, int target_waves, int interleave, int grp, int *out /*[ctiles]*/) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, target_waves, &pl, g_tune)) return -1;
    HadiSweepArgs a{};
    a.L = pl.L; a.ctiles = pl.ctiles; a.btpw = pl.btpw; a.bgroups = pl.bgroups; a.tile_il = interleave;
    if (grp >= pl.bgroups) return -2;
    const HadiTileSet ts = hadi_pb_tiles(a, grp);
    for (int i = 0; i < ts.cnt; i++) out[i] = hadi_pb_tile(ts, i);
    return ts.cnt;
}

// The graph key's view of HadiSweepArgs (hadi_sweep_args_ptrs).  Every 8-byte word of the struct that holds no part of L or of
// an int field is a pointer; each one is set in turn to a value no other field holds, and the helper's list must change.
// Writes the byte offsets of the words whose change the list misses to `out` and returns their number (0: the key sees every
// pointer field).  `nptr_words` receives how many words were probed.
extern "C" int emu_sweep_args_unkeyed(int *out, int cap, int *nptr_words) {
    struct Span { size_t off, len; };
#define HADI_SPAN(f) Span{offsetof(HadiSweepArgs, f), sizeof(HadiSweepArgs::f)}
    const Span ints[] = {HADI_SPAN(L), HADI_SPAN(n_inst), HADI_SPAN(R), HADI_SPAN(ntiles), HADI_SPAN(RS), HADI_SPAN(sblocks),
                         HADI_SPAN(ctiles), HADI_SPAN(btpw), HADI_SPAN(bgroups), HADI_SPAN(tile_il), HADI_SPAN(american),
                         HADI_SPAN(pos_m1), HADI_SPAN(debug)};
#undef HADI_SPAN
    HadiSweepArgs base;
    std::memset(&base, 0, sizeof base);
    const void *p0[HADI_SWEEP_ARGS_NPTRS];
    hadi_sweep_args_ptrs(base, p0);
    int bad = 0, words = 0;
    for (size_t off = 0; off + 8 <= sizeof(HadiSweepArgs); off += 8) {
        bool other = false;
        for (const Span &s : ints) other = other || (off < s.off + s.len && s.off < off + 8);
        if (other) continue;
        words++;
        HadiSweepArgs b = base;
        const unsigned long long v = 0x5000 + off;
        std::memcpy(reinterpret_cast<char *>(&b) + off, &v, 8);
        const void *p1[HADI_SWEEP_ARGS_NPTRS];
        hadi_sweep_args_ptrs(b, p1);
        if (!std::memcmp(p0, p1, sizeof p0)) {
            if (bad < cap) out[bad] = (int)off;
            bad++;
        }
    }
    *nptr_words = words;
    return bad;
}

// the fraction of its CU-rounds the plan's row pass leaves idle (decides one or two streams: hadi_plan_row_idle), x 1e6
extern "C" long long emu_plan_row_idle_ppm(int m1, int m2, int n_inst, int cus) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, 8 * cus, &pl, g_tune)) return -1;
    return (long long)(hadi_plan_row_idle(pl, n_inst, cus) * 1e6 + 0.5);
}

// The host routine that dates the dividends (hadi_plan.h), as the library calls it: flags[n-1] = index paid at the start of step n
// or -1, `len` >= N entries.
extern "C" void emu_dividend_steps(int N, double dt, int ndiv, const double *dates, int *flags, int len) {
    hadi_dividend_steps(N, dt, ndiv, dates, flags, len);
}

// variant bit0 = american, bit1 = dividends.  Arrays natural layout [n][...].
// scheme: 0 Douglas, 1 Craig-Sneyd, 2 Douglas with the fp32 state, 3 Douglas with the American P representation, 4 Modified
// Craig-Sneyd, 5 Hundsdorfer-Verwer.  N_i / dt_i: per-instance time steps and step sizes (NULL: N and dt for every instance);
// the time loop then runs to the largest N_i, as in the library.  Returns 0, 1 (no plan), 2 / 3 (unsupported), 4 (device error
// word set) or 5 (a row pass wrote to an instance after its last step).
extern "C" int emu_solve(int n_inst, int m1, int m2, int N, double dt, double theta, double r_d, double r_f,
                         const double *par /*[n][4] rho sigma kappa eta*/, int variant, const double *vec_s,
                         const double *vec_v, const double *delta_s, const double *delta_v, double *U,
                         const double *U0, double *lam_out, int target_waves, int ndiv, const double *ddates,
                         const double *damounts, const double *dpcts, int setup_threads, int use_small, int scheme,
                         const double *put_strikes /* NULL = call boundary data */, const int *N_i, const double *dt_i) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, n_inst, target_waves, &pl, g_tune, scheme == 2 ? 4 : 8)) return 1;
    if (hadi_no_strips(theta, r_d == r_f)) pl.use_strip = 0;  // (the strip kernels divide by theta dt)
    const HadiLayout &L = pl.L;
    const int american = variant & 1, dividend = (variant >> 1) & 1;
    const size_t st = (size_t)L.inst_stride * n_inst;
    const int hscheme = scheme == 1 ? 1 : scheme == 4 ? 2 : scheme == 5 ? 3 : 0;  // enum hadi_scheme
    const bool cs = hscheme != 0, f32 = scheme == 2, amp = scheme == 3;
    if (scheme < 0 || scheme > 5) return 3;
    if (amp && !american) return 3;
    if (f32 && (american || dividend)) return 3;
    if (cs && (american || dividend || put_strikes)) return 3;  // (the library's predictor-corrector schemes: European calls)
    if (hscheme >= 2 && !(theta > 0.0)) return 3;
    if ((N_i || dt_i) && (!N_i || !dt_i || dividend)) return 3;  // (per-instance step grids: no per-instance dividend tables here)
    int Nmax = N;
    if (N_i) {
        Nmax = 0;
        for (int k = 0; k < n_inst; k++) Nmax = N_i[k] > Nmax ? N_i[k] : Nmax;
    }
    std::vector<double> dV(cs ? st : 0), dR1(cs ? st : 0), dC2(cs ? st : 0);
    std::vector<double> dU(st), dY(st, 0.0), dLAM(american ? st : 0), dU0(american ? st : 0), dUT(dividend ? st : 0);
    std::vector<double> scoef(pl.n_scoef * n_inst), b2row(pl.n_b2row * n_inst), rowc(pl.n_rowc * n_inst),
        a2i(pl.n_a2i * n_inst), pb(pl.n_pb * n_inst), rinv(pl.n_rinv * n_inst), rwork(pl.n_rwork * n_inst);
    std::vector<HadiInstPar> ipar(n_inst);
    std::vector<double> par8((size_t)n_inst * 8);
    for (int k = 0; k < n_inst; k++) {
        for (int z = 0; z < 4; z++) par8[(size_t)k * 8 + z] = par[(size_t)k * 4 + z];
        par8[(size_t)k * 8 + 4] = dt_i ? dt_i[k] : dt;
        par8[(size_t)k * 8 + 5] = (double)(N_i ? N_i[k] : N);
        par8[(size_t)k * 8 + 6] = put_strikes ? put_strikes[k] : 0.0;
        par8[(size_t)k * 8 + 7] = put_strikes ? 1.0 : 0.0;
    }
    HadiSetupArgs s;
    s.L = L; s.n_inst = n_inst;
    s.vec_s = vec_s; s.vec_v = vec_v; s.delta_s = delta_s; s.delta_v = delta_v;
    s.par = par8.data(); s.r_d = r_d; s.r_f = r_f; s.theta = theta;
    s.scoef = scoef.data(); s.b2row = b2row.data(); s.rowc = rowc.data(); s.a2i = a2i.data();
    s.pb = pb.data(); s.rinv = rinv.data(); s.rwork = rwork.data(); s.ipar = ipar.data();
    emu::launch(n_inst, setup_threads, [&]() { hadi_setup_kernel(s); });

    emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U, dU.data()); });
    if (american) {
        emu::launch(8, 64, [&]() { hadi_pack_kernel(L, n_inst, n_inst, U0 ? U0 : U, dU0.data()); });
        emu::launch(8, 64, [&]() { hadi_fill_kernel(dLAM.data(), st, 0.0); });
    }
    HadiSweepArgs a;
    a.U = dU.data(); a.Y = dY.data(); a.LAM = american ? dLAM.data() : nullptr; a.U0 = american ? dU0.data() : nullptr;
    a.scoef = scoef.data(); a.b2row = b2row.data(); a.rowc = rowc.data(); a.pb = pb.data(); a.rinv = rinv.data();
    a.ipar = ipar.data(); a.L = L; a.n_inst = n_inst; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw; a.bgroups = pl.bgroups; a.tile_il = g_tile_il;
    a.american = american; a.pos_m1 = pl.pos_m1; a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = &g_err; a.debug = g_debug;
    std::vector<int> pay_mis(n_inst, 0);
    a.pay_mis = american ? pay_mis.data() : nullptr;
    if (american) emu::launch(8, 64, [&]() { hadi_payoff_shape_kernel(L, n_inst, dU0.data(), pay_mis.data()); });
    std::vector<double> dW(pl.row_seq ? st : 0);
    a.R1 = cs ? dR1.data() : pl.row_seq ? dW.data() : nullptr; a.C2 = cs ? dC2.data() : nullptr;
    const bool pair_tab = hadi_pair_table(pl, cs) && pl.use_strip;  // the pairs' coupling column, built once
    std::vector<double> dRS(pair_tab ? (size_t)n_inst * pl.L.nrows * 128 : 0, std::nan(""));
    a.rs_tab = pair_tab ? dRS.data() : nullptr;
    HadiSweepArgs av = a;
    if (cs) av.U = dV.data();

    std::vector<int> flags(Nmax, -1);
    if (dividend) hadi_dividend_steps(N, dt, ndiv, ddates, flags.data(), N);
    if (use_small == 4) {  // instance-resident launch (hadi_team_kernel) with teams of ONE block: the emulator runs the blocks of a
                           // grid one after the other, so the team barrier is trivially met; indexing and arithmetic are real
        if (american || cs || f32 || !hadi_team_grid(pl, n_inst, theta, r_d == r_f)) return 3;  // (the team kernel's row step is the strips')
        std::vector<int> team(512, 0);
        HadiTeamArgs ta;
        // "team_blocks" > 1: teams of several blocks, all blocks of the grid running at once (the team barrier, the formation
        // counters and the row / column-tile split over the blocks are then real); 1: block after block, a team per block
        const int nb = g_team_blocks;
        ta.form = team.data(); ta.bar = team.data() + 64; ta.nb = nb; ta.N = Nmax; ta.stamps = nullptr;
        ta.div_flag = dividend ? flags.data() : nullptr; ta.flag_stride = 0; ta.div_amounts = damounts; ta.div_pcts = dpcts; ta.vec_s = vec_s;
        const size_t smem = hadi_team_smem(L, dividend != 0);
        if (L.B == 8) emu::launch(8 * nb, 512, [&]() { hadi_team_kernel<8>(a, ta); }, smem, nb > 1);
        else emu::launch(8 * nb, 512, [&]() { hadi_team_kernel<4>(a, ta); }, smem, nb > 1);
        emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U); });
        return g_err ? 4 : 0;
    }
    if (use_small && !cs && !f32 && (american ? pl.smem_small_am : pl.smem_small_eu) > 0) {
        HadiSmallArgs sm;
        sm.div_flag = dividend ? flags.data() : nullptr; sm.flag_stride = 0; sm.div_amounts = damounts; sm.div_pcts = dpcts;
        sm.vec_s = vec_s; sm.Nmax = Nmax; sm.order = nullptr;
        // use_small 5: two instances per wavefront; 3: one wavefront per instance, sequential line solves (both European /
        // dividends); 2: 8 wavefronts per instance (what hadi_api.hip picks for small batches); else 4
        const int kind = (use_small == 5 && !american && pl.L.nrows <= 32) ? 2 : (use_small == 3 && !american) ? 1 : 0;
        const HadiSel sel = hadi_select_small(pl, n_inst, kind, use_small == 2 ? 8 : 4, american != 0);
        if (!sel.k) return 2;
        emu::launch(sel.grid, sel.block, [&]() { sel.k->loop(a, sm); }, sel.smem);
        emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U); });
        if (american && lam_out) emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dLAM.data(), lam_out); });
        return 0;
    }
    if (pair_tab && run_pass(hadi_select_pair_table(pl), a, 1)) return 2;  // (before any sweep of the streaming path, as hadi_api.hip does at the start of a sub-batch's time loop)
    std::vector<float> fU(f32 ? st : 0), fY(f32 ? st : 0, 0.0f);
    if (f32) {  // round the packed state to float, sweep on float arrays, widen again
        emu::launch(8, 64, [&]() { hadi_narrow_kernel(L, dU.data(), fU.data(), st); });
        a.U = reinterpret_cast<double *>(fU.data());
        a.Y = reinterpret_cast<double *>(fY.data());
    }
    // per-instance step grids: an instance that has taken its last step gets NaN in its slices of the arrays the row passes write
    // (Y, R1, C2); a later row pass that still worked on it would overwrite them, a later column pass would carry the NaN into U
    auto poison_finished = [&](int n) {
        for (int k = 0; N_i && k < n_inst; k++) {
            if (N_i[k] != n || n == Nmax) continue;
            for (double *arr : {dY.data(), cs ? dR1.data() : nullptr, cs ? dC2.data() : nullptr})
                if (arr) std::fill(arr + (size_t)k * L.inst_stride, arr + (size_t)(k + 1) * L.inst_stride, std::nan(""));
        }
    };
    for (int n = 1; n <= Nmax; n++) {
        const bool xstep = amp && (n == 1 || (dividend && flags[n - 1] >= 0));  // explicit (U, lambda_bar) step, as in hadi_api.hip
        if (xstep && n > 1)
            emu::launch(8, 64, [&]() { hadi_am_materialise_kernel(L, n_inst, ipar.data(), dU0.data(), dU.data(), dLAM.data(), pl.pos_m1); });
        if (dividend && flags[n - 1] >= 0) {  // device_solver.hpp:426-517 (host builds the step table, kernel applies)
            dUT = dU;
            emu::launch(8, 64, [&]() {
                hadi_dividend_kernel(L, n_inst, ipar.data(), vec_s, dUT.data(), dU.data(), flags.data(), 0, n, damounts, dpcts);
            });
        }
        const HadiPassCtx pc{pl, n_inst, american != 0, amp, xstep, f32, hscheme, g_cs_strips, g_col_prefetch};
        const HadiSel col = hadi_select_col_pass(pc);
        if (col.k && col.k->family == HADI_F_COL_SEQ && (f32 || amp)) return 2;
        for (int mode = cs ? 1 : 0; mode <= (cs ? 2 : 0); mode++) {  // (predictor: V = Y2 out of U; corrector: U out of V)
            const HadiSel row = hadi_select_row_pass(pc, mode);
            // (the library never launches the sequential passes but for Douglas sweeps with the fp64 state: run_sweep refuses)
            if (row.k && row.k->family == HADI_F_ROW_SEQ && (mode || f32 || amp)) return 2;
            if (run_pass(row, mode == 2 ? av : a, n) || run_pass(col, mode == 1 ? av : a, n)) return 2;
        }
        if (xstep)
            emu::launch(8, 64, [&]() { hadi_am_dematerialise_kernel(L, n_inst, ipar.data(), dU0.data(), dU.data(), dLAM.data()); });
        poison_finished(n);
    }
    for (int k = 0; N_i && k < n_inst; k++) {
        if (N_i[k] >= Nmax) continue;
        for (double *arr : {dY.data(), cs ? dR1.data() : nullptr, cs ? dC2.data() : nullptr})
            for (size_t e = 0; arr && e < (size_t)L.inst_stride; e++)
                if (!std::isnan(arr[(size_t)k * L.inst_stride + e])) return 5;  // a row pass ran past the instance's N
    }
    if (amp)
        emu::launch(8, 64, [&]() { hadi_am_materialise_kernel(L, n_inst, ipar.data(), dU0.data(), dU.data(), dLAM.data(), pl.pos_m1); });
    if (f32) emu::launch(8, 64, [&]() { hadi_widen_kernel(L, fU.data(), dU.data(), st); });
    emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dU.data(), U); });
    if (american && lam_out) emu::launch(8, 64, [&]() { hadi_unpack_kernel(L, n_inst, dLAM.data(), lam_out); });
    return 0;
}

// Tables only (serial host evaluation of hadi_setup_instance), for direct comparison with the oracle.
extern "C" int emu_tables(int m1, int m2, int N, double dt, double theta, double r_d, double r_f, double rho,
                          double sigma, double kappa, double eta, const double *vec_s, const double *vec_v,
                          const double *delta_s, const double *delta_v, int target_waves, double *scoef,
                          double *b2row, double *rowc, double *a2i, double *pb, double *rinv) {
    HadiPlan pl;
    if (hadi_make_plan(m1, m2, 1, target_waves, &pl, g_tune)) return 1;
    HadiSetupIn in;
    in.vec_s = vec_s; in.vec_v = vec_v; in.delta_s = delta_s; in.delta_v = delta_v;
    in.r_d = r_d; in.r_f = r_f; in.rho = rho; in.sigma = sigma; in.kappa = kappa; in.eta = eta;
    in.theta = theta; in.dt = dt; in.N = N;
    in.put = 0; in.strike = 0.0;
    std::vector<double> rwork(pl.n_rwork);
    HadiInstPar ip;
    HadiTables t;
    t.scoef = scoef; t.b2row = b2row; t.rowc = rowc; t.a2i = a2i; t.pb = pb; t.rinv = rinv;
    t.rwork = rwork.data(); t.ipar = &ip;
    hadi_setup_instance(pl.L, in, t, 0, 1, HadiNoSync());
    return 0;
}
