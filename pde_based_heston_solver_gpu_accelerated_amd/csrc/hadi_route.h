// hadi_route.h -- which route a whole call takes: the handle's tuning words, how the batch is cut into sub-batches and streams,
// which whole-loop kernel or which streaming path runs it, which buffers it needs, whether its time loop is replayed from a
// graph, and the words of hadi_describe_last_sweep for all of it -- each written once.  run_sweep (hadi_api.hip) consumes the
// route, the wave emulator (tests/emu: emu_route) returns it for given inputs, tests/golden/route_selection.json pins it.
// No HIP runtime calls here: the header compiles under hipcc and under g++ -DHADI_EMU.  The rules: DESIGN.md section 4.1.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "../../include/hadi.h"
#include "hadi_dispatch.h"

// ---- the handle's tuning words (hadi_set_tuning / hadi_get_tuning) -----------------------------------------------------------
struct HadiHandleTuning {
    int use_graph = 1;
    int graph_max_melems = 8;  // hipGraph replay for batches of up to this many Mi state elements
    int use_small = 1;         // LDS-resident one-launch path for small grids
    int small_seq = -1;        // ... European / dividend sweeps on the one-wavefront-per-instance kernel: -1 by batch size, 0 never, 1 always
    int small_pairs = -1;      // small-grid sequential kernel with two instances per wavefront: -1 by batch size, 0 never, 1 always
    int small_sch = -1;        // predictor-corrector schemes on the one-wavefront-per-instance LDS kernel (hadi_small_sch_kernel): -1 by batch size, 0 never, 1 wherever admitted
    int use_amp = 1;           // American sweeps without the lambda_bar array when the payoff depends on s only
    int sub_batch = 1;         // large batches run sub-batch by sub-batch (hadi_plan_batches)
    int streams = 0;           // 0 automatic (hadi_plan_row_idle), 1 one stream, 2 two streams side by side
    int cs_strips = 1;         // Craig-Sneyd row passes on the barrier-free strips where the plan chose strips (0: shared ring, as before round 4)
    // Two measured alternatives of the column pass, both opt-in (round 4; neither moves the 16-chunk pass by more than +-2 %:
    // profiles/r04_colpass_ab.txt): the blocks of an instance take their full column tiles interleaved (hadi_pb_tiles), and
    // hadi_pass_b2 -- part of the next tile prefetched into LDS -- instead of hadi_pass_b1 for European sweeps of 9 .. 16 chunks
    int tile_il = 0;
    int col_prefetch = 0;
    int team_launch = -1;      // instance-resident launch (hadi_team_kernel): -1 automatic, 0 never, 1 whenever the shape allows it
    int resident_sweep = -1;   // resident sweep (hadi_sweep_resident: both passes of every step in one launch, one block per instance): -1 automatic, 0 never, 1 wherever the sub-batch is eligible
    int debug_fault = 0;       // test hook: HADI_DEBUG_* bits handed to the sweep kernels
    int device_vgrid = 1;      // compute_base_prices / compute_jacobian: v-grids rebuilt per instance on the device
    int jump_share = 1;        // eight-column Bates Jacobian, per-instance matrices: the groups 0 .. 6 of a source instance ride on one staged strip of G
    int jump_small = -1;       // sampled Bates ladder on the whole-loop LDS kernel (hadi_small_jump_kernel): -1 automatic, 0 never, 1 wherever admitted
    HadiTuning tune;           // kernel-selection overrides and the constants of the plan's cost model (hadi_plan.h)
};

// One table of {key, field, normalisation} that hadi_set_tuning and hadi_get_tuning both walk.  f: a word of the handle; tf: a
// word of its HadiTuning.
enum HadiTuneNorm { HADI_TN_BOOL, HADI_TN_TRI, HADI_TN_NONNEG, HADI_TN_ANY, HADI_TN_STREAMS, HADI_TN_CS_STRIPS, HADI_TN_POSITIVE, HADI_TN_WAVES };
struct HadiTuneKey { const char *key; int HadiHandleTuning::*f; int HadiTuning::*tf; int norm; };
static inline const HadiTuneKey *hadi_tuning_key(const char *key) {
    typedef HadiHandleTuning H;
    typedef HadiTuning T;
    static const HadiTuneKey tab[] = {
        {"graph", &H::use_graph, nullptr, HADI_TN_BOOL}, {"small_grid", &H::use_small, nullptr, HADI_TN_BOOL},
        {"small_seq", &H::small_seq, nullptr, HADI_TN_TRI}, {"small_sch", &H::small_sch, nullptr, HADI_TN_TRI},
        {"american_p", &H::use_amp, nullptr, HADI_TN_BOOL}, {"device_vgrid", &H::device_vgrid, nullptr, HADI_TN_BOOL},
        {"sub_batch", &H::sub_batch, nullptr, HADI_TN_BOOL}, {"small_pairs", &H::small_pairs, nullptr, HADI_TN_TRI},
        {"streams", &H::streams, nullptr, HADI_TN_STREAMS}, {"col_prefetch", &H::col_prefetch, nullptr, HADI_TN_BOOL},
        {"cs_strips", &H::cs_strips, nullptr, HADI_TN_CS_STRIPS}, {"graph_max_melems", &H::graph_max_melems, nullptr, HADI_TN_NONNEG},
        {"tile_interleave", &H::tile_il, nullptr, HADI_TN_BOOL}, {"debug_fault", &H::debug_fault, nullptr, HADI_TN_ANY},
        {"team_launch", &H::team_launch, nullptr, HADI_TN_TRI}, {"resident_sweep", &H::resident_sweep, nullptr, HADI_TN_TRI},
        {"jump_share", &H::jump_share, nullptr, HADI_TN_BOOL}, {"jump_small", &H::jump_small, nullptr, HADI_TN_TRI},
        {"strip", nullptr, &T::strip, HADI_TN_TRI}, {"row_tile", nullptr, &T::row_tile, HADI_TN_NONNEG},
        {"strip_blocks", nullptr, &T::strip_blocks, HADI_TN_NONNEG}, {"pair_strips", nullptr, &T::pair_strips, HADI_TN_TRI},
        {"col_groups", nullptr, &T::col_groups, HADI_TN_NONNEG}, {"small_waves", nullptr, &T::small_waves, HADI_TN_WAVES},
        {"model_strip_row_ns", nullptr, &T::strip_row_ns, HADI_TN_POSITIVE}, {"model_ring_row_ps", nullptr, &T::ring_row_ps, HADI_TN_POSITIVE},
        {"model_ring_fixed_ns", nullptr, &T::ring_fixed_ns, HADI_TN_POSITIVE}, {"model_pstrip_row_ns", nullptr, &T::pstrip_row_ns, HADI_TN_POSITIVE},
        {"model_pring_row_ps", nullptr, &T::pring_row_ps, HADI_TN_POSITIVE}, {"model_pring_fixed_ns", nullptr, &T::pring_fixed_ns, HADI_TN_POSITIVE}};
    for (const HadiTuneKey &e : tab)
        if (!strcmp(key, e.key)) return &e;
    return nullptr;
}
static inline int &hadi_tuning_word(HadiHandleTuning &t, const HadiTuneKey &e) { return e.f ? t.*(e.f) : t.tune.*(e.tf); }
static inline int hadi_tuning_word(const HadiHandleTuning &t, const HadiTuneKey &e) { return e.f ? t.*(e.f) : t.tune.*(e.tf); }
// Stores the normalised value; returns 0, or the text of the refusal ("%s": the key).
static inline const char *hadi_tuning_set(HadiHandleTuning &t, const HadiTuneKey &e, int v) {
    switch (e.norm) {
        case HADI_TN_BOOL: v = v ? 1 : 0; break;
        case HADI_TN_TRI: v = v < 0 ? -1 : (v ? 1 : 0); break;
        case HADI_TN_NONNEG: v = v > 0 ? v : 0; break;
        case HADI_TN_STREAMS: v = v == 2 ? 2 : (v == 1 ? 1 : 0); break;
        case HADI_TN_CS_STRIPS: v = (v >= 0 && v <= 3) ? v : 1; break;
        case HADI_TN_POSITIVE: if (v < 1) return "%s must be positive"; break;
        case HADI_TN_WAVES: if (v != 0 && v != 4 && v != 8) return "%s must be 0, 4 or 8"; break;
        default: break;
    }
    hadi_tuning_word(t, e) = v;
    return nullptr;
}

// ---- what the route depends on beyond the plan ---------------------------------------------------------------------------------
struct HadiRouteIn {
    int cu_count = 256;
    int n = 0, m1 = 0, m2 = 0;                // instances actually solved (6x the caller's for a Jacobian) and the grid
    int variant = 0, scheme = 0, prec = 0;    // enum hadi_variant, hadi_scheme, hadi_state_precision
    double theta = 0;
    bool rates_equal = false;                 // r_d == r_f
    int debug = 0;                            // diagnostics (hadi_debug_*): one pass of one step
    bool profiling = false;
    int n_snap = 0;                           // maturity ladder: snapshots asked for
    int n_samp = 0;                           // sampled ladder: samples per instance and snapshot (0: the ladder's one node); a
                                              // sample call is a ladder call -- the route does not depend on this, only its words do
    bool dividends = false;                   // num_dividends > 0
    bool uniform_steps = true;
    bool team_failed = false;                 // a team could not form or a team barrier timed out once on this handle
    int n_ex_steps = 0;                       // Bermudan call: steps at whose end some instance may be exercised (0: not a Bermudan call)
    int n_mon_steps = 0;                      // barrier call: steps at whose end some instance is monitored (0: not a barrier call)
    int n_fix_steps = 0;                      // cliquet call: steps at whose end some instance fixes its strike (0: not a cliquet call)
    bool fix_weights = false;                 // ... and some fixing carries a non-zero weight: the packed payoff is read
    bool jumps = false;                       // Bates call with some a_k = lambda_k dt_k != 0: hadi_jump_kernel at the end of every step
    int jump_sets = 1;                        // ... 3: the nine groups of an eight-column Jacobian -- the route does not depend on this, only its words do
    HadiHandleTuning t;
};

// ---- how the batch is cut -------------------------------------------------------------------------------------------------------
// (the strip kernels scale the A1 action by (1 - theta) / theta and keep the s-convection weights multiplied by
// theta dt (r_d - r_f): hadi_strip_step -- without both, every plan's use_strip is cleared)
static inline bool hadi_no_strips(double theta, bool rates_equal) { return !(theta > 0.0) || rates_equal; }
// Paired strips (Douglas steps) take the pairs' coupling column from a table built once per solve, by the sub-batches on strips.
static inline bool hadi_pair_table(const HadiPlan &pl, bool cs) { return pl.L.G == 2 && !cs && !pl.row_seq; }
struct HadiSubBatch { int off, cnt; HadiPlan pl; int lane; };  // lane: 0 = the handle's stream, 1 = its second stream
struct HadiBatchPlan {
    std::vector<HadiSubBatch> subs;
    bool two_streams = false;
    int fork_before = 0;  // the second stream forks off right before this sub-batch is enqueued
};
// Sub-batches (whole rounds of one instance per CU + the remainder) and the one-or-two-streams decision.  `pl` is the plan of
// the whole batch on entry and the plan the caller sees (layout, table sizes) on exit.  Returns non-zero when a plan failed.
static inline int hadi_plan_batches(const HadiRouteIn &in, HadiPlan &pl, int state_bytes, bool seq_shape, HadiBatchPlan &bp) {
    std::vector<HadiSubBatch> &subs = bp.subs;
    bool &two_streams = bp.two_streams;
    int &fork_before = bp.fork_before;
    const int cu = in.cu_count;
    // Large batches on grids where ONE round of the one-block-per-CU kernels (cu_count instances) already moves more than
    // the 256 MB memory-side cache holds: the two passes of a step then re-use each other's data only while the batch is
    // one round deep (measured at 512x256: 512 instances at once ran the column pass 6 % slower per instance than 256;
    // 384 at once: 0.188 + 0.205 ms per step against 0.173 + 0.177 as 256 + 128).  Instances are independent, so the time
    // loop runs sub-batch by sub-batch -- whole rounds of cu_count instances plus the remainder (a remainder below a
    // quarter round rides with the last full round) -- each with the launch geometry of its own size.
    const bool no_strips = hadi_no_strips(in.theta, in.rates_equal);
    auto plan_for = [&](int cnt, HadiPlan *q) {
        if (hadi_make_plan(in.m1, in.m2, cnt, 8 * cu, q, in.t.tune, state_bytes)) return 1;
        if (no_strips) q->use_strip = 0;
        return 0;
    };
    if (no_strips) pl.use_strip = 0;
    if (in.scheme == HADI_SCHEME_DOUGLAS && !in.debug && in.t.sub_batch && in.n > cu &&
        2ll * cu * pl.L.inst_stride * (long long)state_bytes >= (256ll << 20)) {  // (bytes the sweep streams: 4 per element with the fp32 state)
        const int full = in.n / cu, rem = in.n - full * cu;
        for (int k = 0; k < full; k++) subs.push_back(HadiSubBatch{k * cu, cu, pl, 0});
        if (rem >= cu / 4) subs.push_back(HadiSubBatch{full * cu, rem, pl, 0});
        else subs.back().cnt += rem;
        for (auto &sbt : subs)
            if (plan_for(sbt.cnt, &sbt.pl)) return 1;
        pl = subs[0].pl;  // (what the caller sees: layout and table sizes are the same for every sub-batch)
    } else {
        subs.push_back(HadiSubBatch{0, in.n, pl, 0});
    }
    // Two streams.  Forced (hadi_set_tuning "streams" = 2): the sub-batches alternate between the two streams from the start; a
    // batch that is one sub-batch is cut in two halves for it.  Automatic ("streams" = 0, the default): the LAST sub-batch --
    // the whole batch, or the remainder behind the full rounds -- is cut in two halves that run side by side when its row
    // pass would leave a partial round of CUs idle (hadi_plan_row_idle); the full rounds before it run on one stream.
    // Instances are independent and the two passes of a step stay ordered within their own stream.
    const bool streams_ok = in.scheme == HADI_SCHEME_DOUGLAS && !in.debug && !in.profiling && in.n >= 2 && !seq_shape;
    auto split_last = [&]() -> int {
        const HadiSubBatch last = subs.back();
        const int h0 = (last.cnt + 1) / 2;
        subs.pop_back();
        subs.push_back(HadiSubBatch{last.off, h0, last.pl, 0});
        subs.push_back(HadiSubBatch{last.off + h0, last.cnt - h0, last.pl, 1});
        for (size_t k = subs.size() - 2; k < subs.size(); k++)
            if (plan_for(subs[k].cnt, &subs[k].pl)) return 1;
        return 0;
    };
    if (streams_ok && in.t.streams == 2) {
        if (subs.size() == 1) {
            if (split_last()) return 1;
        } else {
            for (size_t k = 0; k < subs.size(); k++) subs[k].lane = (int)(k & 1);
        }
        two_streams = true;
        fork_before = 0;
    } else if (streams_ok && in.t.streams == 0 && subs.back().cnt >= 2 &&
               hadi_plan_row_idle(subs.back().pl, subs.back().cnt, cu) >= HADI_TWO_STREAM_IDLE) {
        const HadiSubBatch whole = subs.back();
        if (split_last()) return 1;
        if (subs[subs.size() - 2].pl.use_strip && subs.back().pl.use_strip) {
            two_streams = true;
            fork_before = (int)subs.size() - 2;
        } else {  // (a half that falls back to the shared ring: the rounds argument does not carry over -- one stream)
            subs.pop_back();
            subs.back() = whole;
        }
    }
    // Several sub-batches (whole rounds plus a remainder) and no half-cut above: they alternate between the two streams, as in the
    // forced mode -- the remainder's launches run in the shadow of a full round's instead of behind it.  Measured on strips
    // (profiles/r04_stream_big.txt): 512x256 x320 +5.1 %, x384 +3.2 %, American x320 / x384 +5.8 / +5.9 %, and within +-1 % from
    // two full rounds on (x512 +0.7 %, x768 -0.3 %, x1024 +0.8 %): never a loss, deterministic per (shape, batch size).
    if (streams_ok && in.t.streams == 0 && !two_streams && subs.size() >= 2) {
        bool strips = true;
        for (auto &sb : subs) strips = strips && sb.pl.use_strip;
        if (strips) {
            for (size_t k = 0; k < subs.size(); k++) subs[k].lane = (int)(k & 1);
            two_streams = true;
            fork_before = 0;
        }
    }
    if (two_streams) pl = subs[0].pl;
    return 0;
}

// ---- eligibility: the parts the emulator's drivers share with the route ----------------------------------------------------------
// Resident sweep (hadi_sweep_resident): European Douglas steps with the fp64 state, 8 nodes per lane on one wavefront per
// v-row, at most 8 column chunks (the grid), and a sub-batch whose strip row pass is ONE block per instance (its plan).
static inline bool hadi_resident_grid(const HadiPlan &pl, double theta, bool rates_equal) {
    return pl.L.B == 8 && pl.L.G == 1 && pl.L.P <= 8 && !pl.row_seq && !pl.col_seq && theta > 0.0 && !rates_equal;
}
static inline bool hadi_resident_plan(const HadiPlan &sp) { return sp.use_strip && !sp.use_pairs && sp.sblocks == 1; }
// Instance-resident launch (hadi_team_kernel): up to 8 instances of a grid with 8 or 4 nodes per lane on one wavefront per
// v-row and at most 8 column chunks; its row step is the strips' (theta > 0, r_d != r_f).
static inline bool hadi_team_grid(const HadiPlan &pl, int n, double theta, bool rates_equal) {
    return n <= 8 && pl.L.G == 1 && (pl.L.B == 8 || pl.L.B == 4) && pl.L.P <= 8 && !pl.row_seq && !pl.col_seq && theta > 0.0 && !rates_equal;
}

// ---- the route ----------------------------------------------------------------------------------------------------------------------
enum HadiRouteKind {
    HADI_ROUTE_SMALL_SCH,   // hadi_small_sch_kernel: whole time loop in one launch, one wavefront per instance
    HADI_ROUTE_SMALL,       // hadi_small_kernel with small_waves wavefronts per instance
    HADI_ROUTE_SMALL_SEQ,   // hadi_small_seq_kernel
    HADI_ROUTE_SMALL_SEQ2,  // hadi_small_seq2_kernel
    HADI_ROUTE_TEAM,        // one attempt at the instance-resident launch, then the streaming path if the team protocol failed
    HADI_ROUTE_STREAMING,   // the time loop over the pass kernels (per sub-batch possibly hadi_sweep_resident)
    HADI_ROUTE_SMALL_JUMP   // hadi_small_jump_kernel with small_waves wavefronts per instance: a sampled Bates ladder in one launch
};
enum { HADI_ROUTE_OK, HADI_ROUTE_BAD_GRID, HADI_ROUTE_SEQ_UNSUPPORTED, HADI_ROUTE_PLAN_FAILED };
enum { HADI_TEAM_NOT_RUN, HADI_TEAM_RAN, HADI_TEAM_FELL_BACK };  // what became of a HADI_ROUTE_TEAM (hadi_describe_route)
struct HadiRoute {
    int status = HADI_ROUTE_OK;
    int kind = HADI_ROUTE_STREAMING;
    int small_waves = 0;         // HADI_ROUTE_SMALL: wavefronts per instance
    HadiPlan pl;                 // what the caller sees: layout and table sizes of every sub-batch
    HadiBatchPlan bp;
    std::vector<char> resident;  // per sub-batch: its whole time loop is one launch of hadi_sweep_resident
    bool american = false, dividend = false, cs = false, f32 = false, seq_shape = false;
    bool ladder = false, prof = false, have_div = false;
    bool bermudan = false;           // exercise steps: the whole-loop LDS kernels or the streaming kernels with hadi_exercise_kernel
    bool barrier = false;            // monitoring steps: the whole-loop LDS kernels or the streaming kernels with hadi_knockout_kernel
    bool cliquet = false;            // fixing steps: the whole-loop LDS kernels or the streaming kernels with hadi_fixing_gather_kernel + hadi_fixing_kernel
    bool jumps = false;              // lognormal jumps: the streaming kernels with hadi_jump_kernel behind every step's last column pass,
                                     // or (a sampled ladder, HADI_ROUTE_SMALL_JUMP) the sub-step inside hadi_small_jump_kernel
    bool read_payoff_shape = false;  // the payoff-shape flags come back to the host: they decide `amp` (filled in by the caller)
    bool pair_tab = false;           // the pairs' coupling table is built
    bool need_u0 = false;            // the packed payoff without a lambda_bar array (a Bermudan call)
    bool need_lam_u0 = false, need_ut = false, need_f32 = false, need_v_r1_c2 = false, need_r1 = false;  // buffers beyond U and Y
    bool graphable = false;          // the time loop may be replayed from a graph
    int n_resident() const { int k = 0; for (char r : resident) k += r; return k; }
};

static inline HadiRoute hadi_route(const HadiRouteIn &in) {
    HadiRoute r;
    const HadiHandleTuning &t = in.t;
    const int state_bytes = in.prec == HADI_STATE_FP32 ? 4 : 8, cu = in.cu_count;
    HadiPlan &pl = r.pl;
    if (hadi_make_plan(in.m1, in.m2, in.n, 8 * cu, &pl, t.tune, state_bytes)) { r.status = HADI_ROUTE_BAD_GRID; return r; }
    const bool seq_shape = r.seq_shape = pl.row_seq || pl.col_seq;  // shapes beyond the streaming kernels: the sequential passes
    if (seq_shape && (in.scheme != HADI_SCHEME_DOUGLAS || in.prec != HADI_STATE_FP64)) { r.status = HADI_ROUTE_SEQ_UNSUPPORTED; return r; }
    if (hadi_plan_batches(in, pl, state_bytes, seq_shape, r.bp)) { r.status = HADI_ROUTE_PLAN_FAILED; return r; }
    const HadiLayout &L = pl.L;
    const bool american = r.american = in.variant == HADI_AM || in.variant == HADI_AM_DIV;
    r.dividend = in.variant == HADI_DIV || in.variant == HADI_AM_DIV;
    const bool cs = r.cs = in.scheme != HADI_SCHEME_DOUGLAS;  // a predictor-corrector scheme (CS, MCS, HV): R1 / C2 carry-over, V = Y2
    const bool f32 = r.f32 = in.prec == HADI_STATE_FP32;      // European Douglas (with or without dividends) only (validated)
    const bool prof = r.prof = in.profiling && !in.debug;
    // A ladder call runs its American sweeps on the explicit (U, lambda_bar) pair (P does not hold U between steps), and it never
    // takes the resident sweep or the team launch -- those sub-batches run the streaming kernels, as under profiling.
    const bool ladder = r.ladder = in.n_snap > 0 && !in.debug;
    // A Bermudan call never takes the resident sweep or the team launch either: its exercise steps sit between two steps of the
    // streaming loop (hadi_exercise_kernel) or inside the whole-loop LDS kernels.
    const bool bermudan = r.bermudan = in.n_ex_steps > 0 && !in.debug;
    // A barrier call (knock-out at the end of its monitoring steps) is kept off both in the same way: hadi_knockout_kernel between
    // two steps of the streaming loop, or the knock-out inside the whole-loop LDS kernels.
    const bool barrier = r.barrier = in.n_mon_steps > 0 && !in.debug;
    // A cliquet call (strike fixings at the end of its fixing steps) likewise: hadi_fixing_gather_kernel and hadi_fixing_kernel
    // between two steps of the streaming loop, or the event inside the whole-loop LDS kernels.
    const bool cliquet = r.cliquet = in.n_fix_steps > 0 && !in.debug;
    // A jump call (Bates) WITHOUT samples takes the streaming path only: the dense sub-step sits between two steps of the streaming
    // loop (hadi_jump_kernel); it is not built into the whole-loop LDS kernels of the table, the resident sweep or the team launch.
    const bool jumps = r.jumps = in.jumps && !in.debug;
    r.have_div = r.dividend && in.dividends && !in.debug;  // (diagnostics take p->U as the state the pass starts from)
    // (a caller who pins the streaming kernels' geometry -- hadi_set_tuning "strip", "row_tile", "col_groups", "strip_blocks" --
    // gets those kernels: no whole-loop kernel, resident sweep or team launch is chosen automatically)
    const bool pinned = t.tune.strip >= 0 || t.tune.row_tile > 0 || t.tune.col_groups > 0 || t.tune.strip_blocks > 0;
    // Predictor-corrector sweeps of grids that fit in LDS (m1 <= 128, m2 <= 32): the whole time loop in one launch, one
    // wavefront per instance (hadi_small_sch_kernel).  "small_sch" = 1: wherever admitted; 0: never; -1 (default): batches of
    // more instances than CUs (the rule of "small_seq") on grids of which a CU's LDS holds at least three instances, unless the
    // caller pinned the streaming geometry or "cs_strips" = 0.  Measured (profiles/r08_small_sch_ab.txt, MCS / HV, ms per step,
    // streaming -> this kernel): 50x25 (three per CU) x257 0.040 -> 0.020, x500 0.057 -> 0.021, x1024 0.082 -> 0.041, x3000
    // 0.210 -> 0.100; 100x30 (one per CU: one wavefront on each CU) x500 0.064 -> 0.081, so such grids stay streaming.
    const bool small_sch = cs && t.use_small && !in.profiling && !in.debug && !t.debug_fault && !f32 && in.variant == HADI_EU &&
                           !seq_shape && hadi_small_sch_admits(L) && !jumps &&
                           (t.small_sch > 0 || (t.small_sch < 0 && in.n > cu && 3 * hadi_small_sch_smem(L) <= (size_t)160 * 1024 &&
                                                !pinned && t.cs_strips != 0));
    // ---- small grids: the whole instance fits in LDS -> one launch runs the entire time loop ----------
    const bool takes_small_path = t.use_small && !in.profiling && !cs && !f32 && !in.debug && !jumps && (american ? pl.smem_small_am : pl.smem_small_eu) > 0;
    // European / dividend sweeps: one wavefront per instance with sequential line solves (hadi_small_seq_kernel) issues about
    // half the instructions per instance and step but runs them on ONE wavefront -- ahead once there are more instances than
    // CUs (50x25, 40 steps, ms block kernel / this one: 256 instances 0.49 / 0.55, 320: 0.67 / 0.60, 512: 0.71 / 0.63, 768: 0.95 /
    // 0.80; 3000 x 50 steps: 3.75 / 2.13), behind below that (a single instance: 10 against 12 us per step).
    // "small_seq" = 1 forces it, 0 forbids it, -1 (default) picks by batch size.
    const bool seq = takes_small_path && !american && (t.small_seq > 0 || (t.small_seq < 0 && in.n > cu));
    // ... and two instances per wavefront for batches of more than 2 and at most 4.5 instances per CU: a wavefront then retires
    // two instances' steps in 1.15x the time of one, but the launch has half the wavefronts -- below 2 per CU the instances are
    // better spread over the CUs, at the 6 per CU that the LDS holds either way the halved instruction count and the halved
    // latency hiding cancel (50x25 x 200 steps, ms: 768 instances 3.20 -> 2.76, 1024: 3.49 -> 2.78, 1536: 3.53 -> 3.83, 3072:
    // 6.68 -> 6.98).  "small_pairs" = 1 forces it, 0 forbids it, -1 (default) picks by batch size.  Needs nrows <= 32.
    const bool seq2 = seq && L.nrows <= 32 && 2 * hadi_small_seq_smem(L) <= (size_t)160 * 1024 &&
                      (t.small_pairs > 0 || (t.small_pairs < 0 && in.n > 2 * cu && 2 * in.n <= 9 * cu));
    // wavefronts per instance of the block kernel: 4 when the batch fills the GPU (throughput), 8 for small batches (latency of
    // the dependent per-step phases; more waves share the rows of the row pass)
    // (measured, 50x25 grid: 1 instance x 100 steps 1.27 -> 1.04 ms with 8; 3000 instances x 50 steps 4.19 -> 4.58 ms)
    r.small_waves = t.tune.small_waves ? t.tune.small_waves : (in.n <= 2 * cu ? 8 : 4);
    // American in the P representation (hadi_row_step, AMER == 2): every payoff of the batch must depend on s only.
    // One small device-to-host copy per solve decides it.
    r.read_payoff_shape = american && t.use_amp && !cs && !takes_small_path && !in.debug && !seq_shape && !ladder;
    r.need_lam_u0 = american;
    r.need_u0 = (bermudan || (cliquet && in.fix_weights)) && !american;
    // A jump call WITH samples (a Bates surface: 1 or 9 instances per source on a calibration grid for ~100 steps) may take
    // hadi_small_jump_kernel, the block kernel of the small path with the sub-step inside its time loop: Douglas steps, fp64 state,
    // European or dividend sweeps, no profiling, no diagnostics, a grid the block kernel admits; never the one-wavefront
    // sequential kernels, whatever n; not when the caller pinned the streaming geometry or switched "small_grid" off.
    // "jump_small" = 1: wherever admitted; 0: never; -1 (default): batches of at least one instance per CU.  Measured
    // (profiles/bates_surface_ab.txt, 100 steps, ms per call, streaming -> this kernel): one 50x25 instance 1.68 -> 1.94 and nine
    // 1.74 -> 1.95, one 100x20 instance 1.98 -> 3.63 -- the replayed graph of the streaming loop is AHEAD for the surface driver's own
    // batches, which therefore stream --; x256 3.6 -> 2.0, x1024 8.9 -> 6.0, x2048 15.9 -> 10.0 at 50x25 and x256 5.7 -> 4.4 at 100x20:
    // from one instance per CU on the one launch is ahead at every measured size, beyond the spread of the rounds.
    const bool small_jump = jumps && ladder && in.n_samp > 0 && !cs && !f32 && !american && !in.profiling && t.use_small && !pinned &&
                            pl.smem_small_eu > 0 && (t.jump_small > 0 || (t.jump_small < 0 && in.n >= cu));
    r.need_ut = r.dividend || (jumps && !small_jump);  // (the streaming sub-step works out of place: it reads the copy of U it finds there)
    r.need_f32 = f32;
    r.need_v_r1_c2 = cs && !small_sch;  // (hadi_small_sch_kernel keeps V, R1, C2 in LDS)
    r.need_r1 = pl.row_seq != 0;        // (hadi_pass_a_seq parks the Thomas multipliers there)
    r.pair_tab = hadi_pair_table(pl, cs);
    // Resident sweep: a sub-batch of eligible shape and plan in ONE round of CUs with less than HADI_TWO_STREAM_IDLE of them idle
    // -- a block that waited for a second round would wait for a whole time loop.  Other sub-batches of the same call (a small
    // remainder) stay on the streaming kernels.  "resident_sweep" = -1 (default): wherever eligible unless the caller pinned the
    // streaming geometry; 1: wherever eligible; 0: never.
    const bool resident_shape = (t.resident_sweep > 0 || (t.resident_sweep < 0 && !pinned)) && in.scheme == HADI_SCHEME_DOUGLAS &&
                                in.variant == HADI_EU && !f32 && hadi_resident_grid(pl, in.theta, in.rates_equal) && !in.debug &&
                                !t.debug_fault && !prof && !ladder && !bermudan && !barrier && !cliquet && !jumps;  // (test hooks: the streaming kernels they are for)
    for (const HadiSubBatch &sbt : r.bp.subs)
        r.resident.push_back(resident_shape && hadi_resident_plan(sbt.pl) && sbt.cnt <= cu &&
                             hadi_plan_row_idle(sbt.pl, sbt.cnt, cu) < HADI_TWO_STREAM_IDLE);
    // Small batches are launch-bound (2*N dependent launches of a few microseconds each): the loop is replayed from a cached
    // hipGraph.
    r.graphable = t.use_graph && !prof && !in.debug && (long long)in.n * L.inst_stride <= ((long long)t.graph_max_melems << 20);
    // ---- instance-resident launch: up to 8 large European instances, one per XCD, whole time loop in one kernel ----------
    // (hadi_team_kernel; the reference runs every instance's time loop inside one kernel, device_solver.hpp:83-88,226-265).
    // Chosen automatically for batches of up to 8 instances on the full 256-CU device; any failure of the team protocol is
    // recorded by the kernel, checked by the caller, and the batch is solved again on the streaming path.
    const bool team = hadi_team_grid(pl, in.n, in.theta, in.rates_equal) && (in.variant == HADI_EU || in.variant == HADI_DIV) && !cs && !f32 &&
                      !in.debug && !prof && cu == 256 && !ladder && !bermudan && !barrier && !cliquet && !jumps && (t.team_launch > 0 || (t.team_launch < 0 && !in.team_failed && !pinned));
    r.kind = small_jump ? HADI_ROUTE_SMALL_JUMP : small_sch ? HADI_ROUTE_SMALL_SCH : takes_small_path ? (seq2 ? HADI_ROUTE_SMALL_SEQ2 : seq ? HADI_ROUTE_SMALL_SEQ : HADI_ROUTE_SMALL) :
             team ? HADI_ROUTE_TEAM : HADI_ROUTE_STREAMING;
    return r;
}

// ---- the route in words (hadi_describe_last_sweep) --------------------------------------------------------------------------------
// The whole-loop kernel of a small-grid route (null where the table holds no such instantiation: an error for the caller).
static inline HadiSel hadi_route_small_sel(const HadiRoute &r, int n) {
    return hadi_select_small(r.pl, n, r.kind == HADI_ROUTE_SMALL_SEQ2 ? 2 : r.kind == HADI_ROUTE_SMALL_SEQ ? 1 : 0, r.small_waves, r.american);
}
static inline int hadi_route_sch(int scheme) { return scheme == HADI_SCHEME_MCS ? HADI_SCH_MCS : scheme == HADI_SCHEME_HV ? HADI_SCH_HV : HADI_SCH_CS; }
// amp: American sweeps in the P representation (the caller's read-back); team: what became of the team launch.
static inline std::string hadi_describe_route(const HadiRoute &r, const HadiRouteIn &in, bool amp, int team = HADI_TEAM_NOT_RUN) {
    const HadiLayout &L = r.pl.L;
    char buf[384];
    // what a ladder call adds
    const std::string samp_words = "; sampled ladder: " + std::to_string(in.n_snap) + " snapshots x " + std::to_string(in.n_samp) + " samples";
    const std::string ladder_loop = !r.ladder ? "" : in.n_samp > 0 ? samp_words + " evaluated inside the time loop" :
                                    "; maturity ladder: " + std::to_string(in.n_snap) + " snapshots copied inside the time loop";
    const std::string ex_loop = r.bermudan ? "; Bermudan: exercise at the end of " + std::to_string(in.n_ex_steps) + " steps inside the time loop" : "";
    const std::string ex_stream = r.bermudan ? "; Bermudan: hadi_exercise_kernel after each of " + std::to_string(in.n_ex_steps) + " exercise steps" : "";
    const std::string ko_loop = r.barrier ? "; barrier: knock-out at the end of " + std::to_string(in.n_mon_steps) + " steps inside the time loop" : "";
    const std::string ko_stream = r.barrier ? "; barrier: hadi_knockout_kernel after each of " + std::to_string(in.n_mon_steps) + " monitoring steps" : "";
    const std::string fix_loop = r.cliquet ? "; cliquet: strike fixing at the end of " + std::to_string(in.n_fix_steps) + " steps inside the time loop" : "";
    const std::string fix_stream = r.cliquet ? "; cliquet: hadi_fixing_kernel after each of " + std::to_string(in.n_fix_steps) + " fixing steps" : "";
    const std::string ladder_stream = !r.ladder ? "" : in.n_samp > 0 ? samp_words + ", hadi_sample_kernel after each snapshot step" :
                                      "; maturity ladder: " + std::to_string(in.n_snap) + " snapshots, hadi_snap_kernel after each snapshot step";
    if (r.kind == HADI_ROUTE_SMALL_SCH) {
        const int sch = hadi_route_sch(in.scheme);
        snprintf(buf, sizeof buf, "hadi_small_sch_kernel<%d,%s>: whole time loop in one launch, one wavefront per instance, predictor and corrector lines solved sequentially in LDS (%zu B)",
                 L.B, sch == HADI_SCH_MCS ? "MCS" : sch == HADI_SCH_HV ? "HV" : "CS", hadi_small_sch_smem(L));
        return buf + ladder_loop + ex_loop + ko_loop + fix_loop;
    }
    if (r.kind == HADI_ROUTE_SMALL_JUMP) {
        snprintf(buf, sizeof buf, "hadi_small_jump_kernel<%d,%d>: whole time loop in one launch, instance resident in LDS (%zu B)", L.B == 1 ? 1 : 2,
                 r.small_waves == 8 ? 8 : 4, r.pl.smem_small_eu);
        return buf + ladder_loop + "; Bates: jump sub-step on the fp64 matrix core inside the time loop";
    }
    if (r.kind == HADI_ROUTE_SMALL_SEQ2 || r.kind == HADI_ROUTE_SMALL_SEQ || r.kind == HADI_ROUTE_SMALL) {
        const HadiSel sel = hadi_route_small_sel(r, in.n);
        if (r.kind == HADI_ROUTE_SMALL_SEQ2)
            snprintf(buf, sizeof buf, "hadi_small_seq2_kernel<%d>: whole time loop in one launch, two instances per wavefront, lines solved sequentially in LDS (2 x %zu B)", L.B, hadi_small_seq_smem(L));
        else if (r.kind == HADI_ROUTE_SMALL_SEQ)
            snprintf(buf, sizeof buf, "hadi_small_seq_kernel<%d>: whole time loop in one launch, one wavefront per instance, lines solved sequentially in LDS (%zu B)", L.B, hadi_small_seq_smem(L));
        else
            snprintf(buf, sizeof buf, "hadi_small_kernel<%d,%d,%s>: whole time loop in one launch, instance resident in LDS (%zu B)", L.B,
                     sel.k ? sel.k->G : 0, r.american ? "AM" : "EU", sel.smem);
        return buf + ladder_loop + ex_loop + ko_loop + fix_loop;
    }
    if (team == HADI_TEAM_RAN) {
        snprintf(buf, sizeof buf, "hadi_team_kernel<%d>: whole time loop in one launch, every instance resident in one XCD's L2 (teams of %d blocks)",
                 L.B, in.cu_count / 8);
        return buf;
    }
    // the kernels of the streaming path, its sub-batches and streams
    const std::vector<HadiSubBatch> &subs = r.bp.subs;
    const int nsub = (int)subs.size();
    hadi_describe_passes(HadiPassCtx{r.pl, in.n, r.american, amp, false, r.f32, in.scheme, in.t.cs_strips, in.t.col_prefetch}, buf, sizeof buf);
    std::string s = buf;
    if (nsub > 1) {
        bool same = true;
        for (auto &sbt : subs) same = same && sbt.cnt == subs[0].cnt;
        if (same) s += "; " + std::to_string(nsub) + " sub-batches of " + std::to_string(subs[0].cnt) + " instances";
        else {
            s += "; " + std::to_string(nsub) + " sub-batches of";
            for (auto &sbt : subs) s += " " + std::to_string(sbt.cnt);
            s += " instances (each with the geometry of its own size)";
        }
        if (r.bp.two_streams && r.bp.fork_before > 0) s += ", the last two side by side on two streams";
        else if (r.bp.two_streams) s += ", side by side on two streams";
    }
    const int nres = r.n_resident();
    if (nres == nsub)
        s += "; both passes of every step in one launch: hadi_sweep_resident<8> (one block per instance, all column tiles)";
    else if (nres)
        s += "; both passes of every step in one launch for " + std::to_string(nres) +
             " sub-batches of one round: hadi_sweep_resident<8> (one block per instance, all column tiles), the others streaming";
    s += ladder_stream;
    s += ex_stream;
    s += ko_stream;
    s += fix_stream;
    if (r.jumps && in.jump_sets > 1) s += "; Bates: hadi_jump_sel_kernel (fp64 matrix core, three matrix sets picked by group) behind the last column pass of every step";
    else if (r.jumps) s += "; Bates: hadi_jump_kernel (fp64 matrix core) behind the last column pass of every step";
    if (team == HADI_TEAM_FELL_BACK) s += " (after a failed instance-resident launch)";
    return s;
}
