// hadi_api.hip -- host side of libhadi: handle, HBM buffers, launches.  C ABI in include/hadi.h.
// There is deliberately no CPU compute path in this file: without a GPU hadi_create fails.
#include "../../include/hadi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "hadi_route.h"

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> kev;  // per-launch events (profiling)
    int profiling = 0;
    int cu_count = 256;
    std::string name, arch;
    std::string err;
    hadi_timing timing{};
    // grow-only device buffers
    DevBuf U, Y, LAM, U0, UT;
    DevBuf V, R1, C2;                 // Craig-Sneyd: predictor result and carry-over arrays
    DevBuf rs_tab;                    // paired strips: the pairs' coupling column behind the cyclic reduction, per (instance, v-row, half, lane)
    DevBuf Uf, Yf;                    // fp32-state sweep: the two state arrays as float
    DevBuf scoef, b2row, rowc, a2i, pb, rinv, rwork, ipar, par8;
    DevBuf g_s, g_v, g_ds, g_dv;      // grids owned by the library (staged / broadcast)
    DevBuf src_v, src_dv, sel_a, sel_b, v0_i;
    DevBuf natU, natU0, natOut, prices, status;
    // hipGraph cache for the time loop (2 launches per step: launch-bound for small batches)
    struct GraphEntry { std::string key; hipGraph_t graph; hipGraphExec_t exec; unsigned long long stamp; };
    std::vector<GraphEntry> graphs;
    unsigned long long graph_clock = 0;
    // cumulative per handle (hadi_get_tuning "graph_captures" / "graph_replays" / "graph_drops" / "graph_evictions"): time loops
    // captured, replayed from the cache, cache entries destroyed because a buffer was freed (ensure), evicted as least recently used
    unsigned long long graph_captures = 0, graph_replays = 0, graph_drops = 0, graph_evictions = 0;
    HadiHandleTuning t;  // the tuning words (hadi_set_tuning; csrc/hadi_route.h)
    hipStream_t stream2 = nullptr;                 // the second stream of a two-stream sweep
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    int last_nsub = 1;
    hipEvent_t wait_ev = nullptr;  // hadi_wait_stream
    DevBuf lm31;
    std::string last_path;  // which kernels the last sweep ran (hadi_describe_last_sweep)
    DevBuf div_flag, div_amt, div_pct;
    DevBuf pay_mis;  // American: per-instance payoff-shape flags (hadi_payoff_shape_kernel)
    DevBuf order;    // small-grid path: dispatch order of the instances (multi-maturity batches)
    DevBuf ex_flag;  // Bermudan: the exercise table, one row of Nmax flags (shared) or one per instance
    // knock-out barrier: the monitoring table (as ex_flag), the bounds [n][2], the live index ranges [n][2] (hadi_barrier_locate_kernel)
    // and the rebates [n]
    DevBuf ko_flag, ko_bounds, ko_iab, ko_rebate;
    // strike fixings (cliquet calls): the fixing table (as ex_flag) and the weights' table of the same shape and stride, the reference
    // spots [n], their nodes [n] with the status words [n] behind them (hadi_fixing_locate_kernel), the modes [n] and the gathered
    // reference values c [n][nrows_pad] of the streaming path (hadi_fixing_gather_kernel)
    DevBuf fix_flag, fix_w, fix_ref, fix_iref, fix_mode, fix_c;
    // lognormal jumps (Bates calls): the generators in operand order [n_mat][hadi_jump_matrix_doubles] (hadi_jump_matrix_kernel), the
    // weights a_k = lambda_k dt_k [n], the (mu, sigma) pairs of the matrices [n_mat][2], the status word of the shared-grid promise
    DevBuf jmp_G, jmp_a, jmp_par, jmp_stat;
    DevBuf jmp_mat;  // hadi_small_jump_kernel: every instance's matrix index [n]
    DevBuf snap_steps, snap_node, snap_out;  // maturity ladder: the snapshot steps, the instances' price nodes, the snapshots [n][n_snap]
    // sampled ladder: the spots [n][n_samp] and behind them the scales [n][n_samp] as staged; the tap records [n][n_samp] and behind
    // them the samples' flag words [n][n_samp] (hadi_sample_locate_kernel); the samples [n][n_snap][n_samp]
    DevBuf samp_in, samp_tap, samp_out;
    // Sticky device error word: one int in host-pinned, device-visible memory.  Kernels OR a HADI_DEVERR_* code into it
    // (system-scope atomic, only ever on a failure path); finish_timing reads it after the stream synchronisation every
    // entry point ends with -- no copy, no extra launch -- and turns a non-zero word into HADI_ERR_INTERNAL.
    int *err_host = nullptr, *err_dev = nullptr;
    // Pinned staging arena for the small host-side vectors of a call (per-instance parameters, dividend tables, dispatch order,
    // selectors, status words).  A copy out of pageable memory blocks the host and its source has to outlive it -- every such
    // vector used to cost a stream synchronisation in the middle of a call (three per Jacobian: ~0.15 ms of a 1.7 ms call on
    // the calibration grids).  Copies out of this arena are truly asynchronous; it is rewound at the start of every entry point
    // (each ends with a stream synchronisation, so nothing of the previous call is in flight) and grown there when a call asked
    // for more than it holds (the request that did not fit takes the old copy-and-synchronise path once).
    char *pin = nullptr;
    size_t pin_cap = 0, pin_used = 0, pin_want = 0;
    int pin_dirty = 0;  // copies out of the arena may be in flight (cleared by the stream synchronisation that ends a call)
    int team_failed = 0;  // a team (hadi_team_kernel) could not form or a team barrier timed out once on this handle: the automatic
                          // choice then stays away (hadi_set_tuning "team_launch" clears it)
    DevBuf team;
};

// Every GPU entry point runs on the handle's device whatever the caller's current device is (a torch rank that
// never called set_device sits on device 0), and leaves the caller's choice as it found it.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int fail(Ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(c, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((c), HADI_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                      \
    } while (0)

// Destroys every cached time loop (the caller has synchronised the stream: none of them is in flight).
void drop_graphs(Ctx *c) {
    for (auto &g : c->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    c->graph_drops += c->graphs.size();
    c->graphs.clear();
}

// Grows a buffer.  A captured time loop bakes the addresses of the handle's buffers into its nodes, so freeing any of them
// empties the graph cache first: no later call can replay a freed address, whatever the graph key holds.
int ensure(Ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return HADI_OK;
    if (b.p) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        drop_graphs(c);
        HIP_TRY(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, HADI_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return HADI_OK;
}

template <class T>
T *ptr(DevBuf &b) {
    return static_cast<T *>(b.p);
}

// Start of an entry point: nothing of the previous call is in flight (it ended with a stream synchronisation).
void pin_rewind(Ctx *c) {
    if (c->pin_dirty && c->stream) (void)hipStreamSynchronize(c->stream);  // (a call that left through an error path)
    c->pin_dirty = 0;
    if (c->pin_want > c->pin_cap) {
        if (c->pin) (void)hipHostFree(c->pin);
        c->pin = nullptr; c->pin_cap = 0;
        const size_t want = c->pin_want + c->pin_want / 2 + 4096;
        void *q = nullptr;
        if (hipHostMalloc(&q, want, hipHostMallocDefault) == hipSuccess) { c->pin = static_cast<char *>(q); c->pin_cap = want; }
    }
    c->pin_used = 0;
    c->pin_want = 0;
}
// `bytes` of pinned staging memory, or nullptr if the arena cannot hold them (the caller then takes the synchronising path).
void *pin_alloc(Ctx *c, size_t bytes) {
    const size_t need = (bytes + 63) & ~(size_t)63;
    c->pin_want += need;
    if (!c->pin || c->pin_used + need > c->pin_cap) return nullptr;
    void *q = c->pin + c->pin_used;
    c->pin_used += need;
    return q;
}
// Host -> device copy of a small host vector: through the pinned arena (asynchronous, the source may die at once), or, if it
// does not fit, straight from the caller's memory followed by a stream synchronisation.
int stage_to_device(Ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return HADI_OK;
    void *q = pin_alloc(c, bytes);
    if (q) {
        std::memcpy(q, src, bytes);
        c->pin_dirty = 1;
        HIP_TRY(c, hipMemcpyAsync(dst, q, bytes, hipMemcpyHostToDevice, c->stream));
        return HADI_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HADI_OK;
}

int grid1d(size_t n) {  // blocks of 256 threads, at most 4096 of them (the kernels stride)
    return (int)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 4096);
}

// ---- host grid code (grid.cpp:16-61, grid_pod.hpp:25-87) ---------------------------------------
void sorted_insert_drop_largest(double *v, int n, double x0) {
    // push_back(x0); sort; pop_back on an ascending array of n values
    if (!(x0 < v[n - 1])) return;
    int pos = 0;
    while (pos < n && v[pos] <= x0) pos++;
    for (int k = n - 1; k > pos; k--) v[k] = v[k - 1];
    v[pos] = x0;
}
void build_v(int m2, double V_0, double V, double d, double *vec_v, double *delta_v) {
    const double Delta_eta = (1.0 / m2) * std::asinh(V / d);
    for (int i = 0; i <= m2; i++) vec_v[i] = d * std::sinh(i * Delta_eta);
    sorted_insert_drop_largest(vec_v, m2 + 1, V_0);
    for (int i = 0; i < m2; i++) delta_v[i] = vec_v[i + 1] - vec_v[i];
}

// ---- one batched sweep ----------------------------------------------------------------------------
// A step schedule as the entry points receive it (exercise steps of a Bermudan call, monitoring steps of a barrier call): steps
// [rows][n_ex], host array, validated (check_bermudan: rows strictly increasing within 1 .. N_k, zero-padded).  rows 1 = one
// schedule for the batch, else one row per source instance (instance k reads row k % n_src: a Jacobian's groups share).
struct ExSched {
    int n_ex = 0, rows = 0;
    const int *steps = nullptr;
};

struct SweepDesc {
    int n = 0;               // instances actually solved (6x the caller's for a Jacobian)
    int m1 = 0, m2 = 0, variant = 0, scheme = 0, prec = 0;
    double theta = 0, r_d = 0, r_f = 0;
    std::vector<double> par8;  // [n][8] rho sigma kappa eta dt N . .
    int Nmax = 0;
    bool uniform_steps = true;
    double dt0 = 0;
    const double *d_vec_s = nullptr, *d_vec_v = nullptr, *d_delta_s = nullptr, *d_delta_v = nullptr;  // device [n][..]
    const double *d_natU = nullptr;   // device natural [n_src][m]
    const double *d_natU0 = nullptr;  // device natural [n_src][m] or null
    int n_src = 0;                    // natural arrays hold n_src instances, instance k reads k % n_src
    int num_div = 0;
    const double *div_dates = nullptr, *div_amounts = nullptr, *div_pcts = nullptr;
    // diagnostics (hadi_debug_*): 1 = only the row pass of step debug_step, 2 = only one column solve of the packed input
    int debug = 0, debug_step = 1;
    // maturity ladder (hadi_maturity_ladder and its launchers): n_snap > 0 = the value of the price node of (S_0, V_0 or v0_i) after
    // each of the steps snap_steps[0 .. n_snap) (host array, strictly increasing, within 1 .. Nmax) goes to Ctx::snap_out
    int n_snap = 0;
    const int *snap_steps = nullptr;
    double S_0 = 0, V_0 = 0;
    const double *d_v0_i = nullptr;  // device [n] or null: per-instance V_0 of the node's v-row
    // sampled ladder (hadi_sample_ladder and its launchers): n_samp > 0 = a ladder call that evaluates n_samp interpolants of the row
    // of V_0 where the ladder copies one node (S_0 is not read).  spots / scales: host [samp_rows][n_samp] (validated; scales may be
    // null = 1); samp_rows 1 = one list for the batch, else one row per source instance (instance k reads row k % n_src)
    int n_samp = 0, samp_rows = 0;
    const double *spots = nullptr, *scales = nullptr;
    // Bermudan (hadi_bermudan_timestepping and its launchers): ex.n_ex > 0 = the steps at whose end an instance takes
    // U <- max(U, payoff).  Knock-out barrier (hadi_barrier_timestepping and its launchers): mon.n_ex > 0 = the steps at whose end an
    // instance is monitored; ko_lower / ko_upper / ko_rebate: host [n_src] or null (validated; null = -inf / +inf / 0), instance k
    // reads entry k % n_src as it reads its schedule's row.
    ExSched ex, mon;
    const double *ko_lower = nullptr, *ko_upper = nullptr, *ko_rebate = nullptr;
    // Strike fixings (hadi_cliquet_timestepping and its launchers): fix.n_ex > 0 = the steps at whose end an instance fixes its
    // strike; fix_ref: host [n_src] (validated); fix_mode: host [n_src] or null (= SHARES); fix_weights: host [fix.rows][fix.n_ex]
    // or null (= 0), parallel to the schedule.  Instance k reads entry / row k % n_src.
    ExSched fix;
    const double *fix_ref = nullptr, *fix_weights = nullptr;
    const int *fix_mode = nullptr;
    // Lognormal jumps (hadi_bates_timestepping and its launchers): jmp_a non-empty = [n] weights a_k = lambda_k dt_k of the sub-step
    // at the end of every step, some of them non-zero (a call whose weights are all zero carries none: it is the plain call);
    // jmp_musig: [jmp_nmat][2], the (mu, sigma) of the matrices -- one per source instance (instance k uses matrix k % n_src), or
    // ONE for the batch with jmp_shared (the caller's promise of a shared s-grid, checked on the device).
    // jmp_sets = 3 (hadi_compute_jacobian_bates_jumps): the batch is 9 groups, and jmp_musig holds three sets of jmp_nmat / 3
    // matrices -- (mu, sigma), (mu + eps, sigma), (mu, sigma + eps) -- that hadi_jump_sel_kernel picks from by group.
    std::vector<double> jmp_a, jmp_musig;
    int jmp_nmat = 0, jmp_sets = 1;
    bool jmp_shared = false;
};

// Kernels whose dynamic LDS can exceed the 64 KiB default need the limit raised once (hadi_create: every kernel of
// hadi_for_each_kernel).
template <class K>
hipError_t raise_lds_limit(K kernel) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// ---- run_sweep: plan and route (csrc/hadi_route.h), grow buffers, stage inputs, then one whole-loop launch or the time loop ----
// What the host keeps of a per-step, per-instance flag table on the device (dividends, exercise, monitoring).
struct StepTable {
    std::vector<char> any;  // step -> some instance's flag is set: the time loop launches the table's kernel at that step
    int stride = 0;         // the device table holds one shared row (0) or a row of Nmax flags per instance
    size_t bytes(const SweepDesc &d) const { return sizeof(int) * (size_t)(stride ? d.n : 1) * d.Nmax; }
};

// Everything the steps below share.  The route is a pure function of `in`; `amp` is the one thing the device decides.
struct Sweep {
    const SweepDesc &d;
    HadiRouteIn in;
    HadiRoute r;
    size_t tot = 0, st = 0;      // the packed state of the whole batch: elements, and bytes as fp64
    StepTable div;               // somebody pays a dividend at the step's start
    StepTable ex;                // somebody may be exercised at the step's end (Bermudan)
    StepTable mon;               // somebody is monitored at the step's end (knock-out barrier)
    StepTable fix;               // somebody fixes its strike at the step's end (cliquet)
    std::vector<int> snap_q;     // step -> snapshot index of a ladder call, or -1
    bool amp = false;            // American sweeps in the P representation (hadi_row_step, AMER == 2)
    HadiSweepArgs a, av;         // whole-batch arguments; Craig-Sneyd: the predictor's column pass writes V (= Y2), the
                                 // corrector's row pass reads V (av.U)
};

HadiRouteIn route_in(const Ctx *c, const SweepDesc &d) {
    HadiRouteIn in;
    in.cu_count = c->cu_count;
    in.n = d.n; in.m1 = d.m1; in.m2 = d.m2; in.variant = d.variant; in.scheme = d.scheme; in.prec = d.prec;
    in.theta = d.theta; in.rates_equal = d.r_d == d.r_f;
    in.debug = d.debug; in.profiling = c->profiling != 0; in.n_snap = d.n_snap; in.n_samp = d.n_samp; in.dividends = d.num_div > 0;
    in.uniform_steps = d.uniform_steps; in.team_failed = c->team_failed != 0; in.t = c->t;
    in.jumps = !d.jmp_a.empty();
    in.jump_sets = d.jmp_sets;
    return in;
}

// The steps of the time loop behind which a schedule's kernel is launched (hadi_exercise_kernel, hadi_knockout_kernel); returns
// their number, for the route.
int mark_steps(const SweepDesc &d, const ExSched &s, StepTable &t) {
    t.any.assign(d.Nmax + 1, 0);
    t.stride = s.rows > 1 ? d.Nmax : 0;
    for (size_t e = 0; e < (size_t)s.rows * s.n_ex; e++)
        if (s.steps[e] > 0) t.any[s.steps[e]] = 1;
    return (int)std::count(t.any.begin(), t.any.end(), (char)1);
}

// The choice, the launch geometry and the words are hadi_dispatch.h's (the rules: DESIGN.md section 4.1); this launches it.
int launch_pass(Ctx *c, const HadiSel &sel, hipStream_t q, const HadiSweepArgs &ar, int nstep) {
    if (!sel.k) return fail(c, HADI_ERR_INTERNAL, "no kernel for this pass (grid %dx%d)", ar.L.m1, ar.L.m2);
    hipLaunchKernelGGL((sel.k->fn), dim3(sel.grid), dim3(sel.block), sel.smem, q, ar, nstep);
    return HADI_OK;
}

int grow_buffers(Ctx *c, Sweep &w) {
    const SweepDesc &d = w.d;
    const HadiRoute &r = w.r;
    const HadiPlan &pl = r.pl;
    const size_t st = w.st, n = d.n;
    int rc;
    if ((rc = ensure(c, c->U, st)) || (rc = ensure(c, c->Y, st))) return rc;
    if (r.need_lam_u0 && ((rc = ensure(c, c->LAM, st)) || (rc = ensure(c, c->U0, st)))) return rc;
    if (r.need_u0 && (rc = ensure(c, c->U0, st))) return rc;
    if (r.bermudan && (rc = ensure(c, c->ex_flag, w.ex.bytes(d)))) return rc;
    if (r.barrier && ((rc = ensure(c, c->ko_flag, w.mon.bytes(d))) || (rc = ensure(c, c->ko_bounds, 16 * n)) ||
                      (rc = ensure(c, c->ko_iab, 2 * sizeof(int) * n)) || (rc = ensure(c, c->ko_rebate, 8 * n))))
        return rc;
    if (r.cliquet && ((rc = ensure(c, c->fix_flag, w.fix.bytes(d))) || (rc = ensure(c, c->fix_w, 2 * w.fix.bytes(d))) ||
                      (rc = ensure(c, c->fix_ref, 8 * n)) || (rc = ensure(c, c->fix_iref, 2 * sizeof(int) * n)) ||
                      (rc = ensure(c, c->fix_mode, sizeof(int) * n)) || (rc = ensure(c, c->fix_c, 8 * n * pl.L.nrows_pad))))
        return rc;
    if (r.jumps && ((rc = ensure(c, c->jmp_G, 8 * (size_t)d.jmp_nmat * hadi_jump_matrix_doubles(pl.L))) || (rc = ensure(c, c->jmp_a, 8 * n)) ||
                    (rc = ensure(c, c->jmp_par, 16 * (size_t)d.jmp_nmat)) || (rc = ensure(c, c->jmp_stat, sizeof(int))) ||
                    (rc = ensure(c, c->jmp_mat, sizeof(int) * n))))
        return rc;
    if (r.need_ut && (rc = ensure(c, c->UT, st))) return rc;
    if (r.need_f32 && ((rc = ensure(c, c->Uf, st / 2)) || (rc = ensure(c, c->Yf, st / 2)))) return rc;
    if (r.need_v_r1_c2 && ((rc = ensure(c, c->V, st)) || (rc = ensure(c, c->R1, st)) || (rc = ensure(c, c->C2, st)))) return rc;
    if (r.need_r1 && (rc = ensure(c, c->R1, st))) return rc;
    if (r.pair_tab && (rc = ensure(c, c->rs_tab, n * pl.L.nrows * 128 * 8))) return rc;
    if ((rc = ensure(c, c->scoef, pl.n_scoef * n * 8)) || (rc = ensure(c, c->b2row, pl.n_b2row * n * 8)) ||
        (rc = ensure(c, c->rowc, pl.n_rowc * n * 8)) || (rc = ensure(c, c->a2i, pl.n_a2i * n * 8)) ||
        (rc = ensure(c, c->pb, pl.n_pb * n * 8)) || (rc = ensure(c, c->rinv, pl.n_rinv * n * 8)) ||
        (rc = ensure(c, c->rwork, pl.n_rwork * n * 8)) || (rc = ensure(c, c->ipar, sizeof(HadiInstPar) * n)) ||
        (rc = ensure(c, c->par8, 8 * 8 * n)))
        return rc;
    // A ladder call: its buffers are grown here, before anything is captured (a grown buffer drops the graph cache).
    w.snap_q.assign(d.Nmax + 2, -1);
    if (r.ladder) {
        if ((rc = ensure(c, c->snap_steps, sizeof(int) * d.n_snap)) || (rc = ensure(c, c->snap_node, sizeof(int) * n)) ||
            (rc = ensure(c, c->snap_out, 8 * n * d.n_snap)) || (rc = ensure(c, c->status, sizeof(int) * n)))
            return rc;
        for (int q = 0; q < d.n_snap; q++) w.snap_q[d.snap_steps[q]] = q;
        const size_t ns = n * d.n_samp;  // a sample call: the staged lists, the tap table with its flag words, the samples
        if (ns && ((rc = ensure(c, c->samp_in, 2 * 8 * ns)) || (rc = ensure(c, c->samp_tap, (sizeof(HadiTap) + sizeof(int)) * ns)) ||
                   (rc = ensure(c, c->samp_out, 8 * ns * d.n_snap))))
            return rc;
    }
    return HADI_OK;
}

// Discrete dividends: host-built table "which dividend does instance k pay at the start of step n" (one shared
// row when the batch has a single (N, delta_t)), plus the set of steps where anybody pays.
int stage_dividends(Ctx *c, Sweep &w) {
    const SweepDesc &d = w.d;
    w.div.any.assign(d.Nmax + 1, 0);
    w.div.stride = d.uniform_steps ? 0 : d.Nmax;
    if (!w.r.have_div) return HADI_OK;
    const int rows = d.uniform_steps ? 1 : d.n;
    std::vector<int> div_flags((size_t)rows * d.Nmax);
    for (int k = 0; k < rows; k++) {
        const double dt = d.par8[(size_t)k * 8 + 4];
        const int N = (int)d.par8[(size_t)k * 8 + 5];
        int *f = div_flags.data() + (size_t)k * d.Nmax;
        hadi_dividend_steps(N, dt, d.num_div, d.div_dates, f, d.Nmax);
        for (int q = 0; q < d.Nmax; q++)
            if (f[q] >= 0) w.div.any[q + 1] = 1;
    }
    int rc;
    if ((rc = ensure(c, c->div_flag, div_flags.size() * sizeof(int))) || (rc = ensure(c, c->div_amt, d.num_div * 8)) ||
        (rc = ensure(c, c->div_pct, d.num_div * 8)))
        return rc;
    if ((rc = stage_to_device(c, c->div_flag.p, div_flags.data(), div_flags.size() * sizeof(int))) ||
        (rc = stage_to_device(c, c->div_amt.p, d.div_amounts, (size_t)d.num_div * 8)) ||
        (rc = stage_to_device(c, c->div_pct.p, d.div_pcts, (size_t)d.num_div * 8)))
        return rc;
    return HADI_OK;
}

// A schedule's table on the device: host-built "does the schedule of instance k list step n" (one shared row for one shared
// schedule) -- may the instance be exercised at the end of the step (Bermudan), is it monitored there (barrier).
int stage_step_flags(Ctx *c, const SweepDesc &d, const ExSched &s, const StepTable &t, DevBuf &table) {
    const int rows = t.stride ? d.n : 1;
    std::vector<int> flags((size_t)rows * d.Nmax, 0);
    for (int k = 0; k < rows; k++) {
        const int *row = s.steps + (size_t)(t.stride ? k % d.n_src : 0) * s.n_ex;
        for (int q = 0; q < s.n_ex; q++)
            if (row[q] > 0) flags[(size_t)k * d.Nmax + row[q] - 1] = 1;
    }
    return stage_to_device(c, table.p, flags.data(), flags.size() * sizeof(int));
}

// Barrier: behind the monitoring table, the bounds and the rebates of all n instances, then the live index ranges from the device
// s-grids (hadi_barrier_locate_kernel).
int stage_barrier(Ctx *c, const Sweep &w) {
    const SweepDesc &d = w.d;
    std::vector<double> bounds((size_t)2 * d.n), rebate(d.n);
    for (int k = 0; k < d.n; k++) {
        const int src = k % d.n_src;
        bounds[2 * (size_t)k] = d.ko_lower ? d.ko_lower[src] : -INFINITY;
        bounds[2 * (size_t)k + 1] = d.ko_upper ? d.ko_upper[src] : INFINITY;
        rebate[k] = d.ko_rebate ? d.ko_rebate[src] : 0.0;
    }
    int rc;
    if ((rc = stage_step_flags(c, d, d.mon, w.mon, c->ko_flag)) ||
        (rc = stage_to_device(c, c->ko_bounds.p, bounds.data(), bounds.size() * 8)) ||
        (rc = stage_to_device(c, c->ko_rebate.p, rebate.data(), rebate.size() * 8)))
        return rc;
    hipLaunchKernelGGL(hadi_barrier_locate_kernel, dim3((d.n + 63) / 64), dim3(64), 0, c->stream, w.r.pl.L, d.n, d.d_vec_s,
                       ptr<double>(c->ko_bounds), ptr<int>(c->ko_iab));
    return HADI_OK;
}

// Cliquet: behind the fixing table, the weights' table (the shape and stride of the fixing table: entry [k][n - 1] is the weight of
// instance k's fixing at step n), the reference spots and the modes of all n instances, then the reference nodes and their status
// words from the device s-grids (hadi_fixing_locate_kernel) -- on every call, also before a replay: they are data.
int *fix_status(Ctx *c, const SweepDesc &d) { return ptr<int>(c->fix_iref) + d.n; }
int stage_cliquet(Ctx *c, const Sweep &w) {
    const SweepDesc &d = w.d;
    const int rows = w.fix.stride ? d.n : 1;
    std::vector<double> wt((size_t)rows * d.Nmax, 0.0), ref(d.n);
    std::vector<int> mode(d.n);
    for (int k = 0; k < rows; k++) {
        const size_t row = (size_t)(w.fix.stride ? k % d.n_src : 0) * d.fix.n_ex;
        for (int q = 0; q < d.fix.n_ex && d.fix_weights; q++)
            if (d.fix.steps[row + q] > 0) wt[(size_t)k * d.Nmax + d.fix.steps[row + q] - 1] = d.fix_weights[row + q];
    }
    for (int k = 0; k < d.n; k++) {
        ref[k] = d.fix_ref[k % d.n_src];
        mode[k] = d.fix_mode ? d.fix_mode[k % d.n_src] : HADI_FIX_SHARES;
    }
    int rc;
    if ((rc = stage_step_flags(c, d, d.fix, w.fix, c->fix_flag)) || (rc = stage_to_device(c, c->fix_w.p, wt.data(), wt.size() * 8)) ||
        (rc = stage_to_device(c, c->fix_ref.p, ref.data(), ref.size() * 8)) ||
        (rc = stage_to_device(c, c->fix_mode.p, mode.data(), mode.size() * sizeof(int))))
        return rc;
    hipLaunchKernelGGL(hadi_fixing_locate_kernel, dim3((d.n + 63) / 64), dim3(64), 0, c->stream, w.r.pl.L, d.n, d.d_vec_s,
                       ptr<double>(c->fix_ref), ptr<int>(c->fix_iref), fix_status(c, d));
    return HADI_OK;
}

// Bates: the weights a_k and the matrices' (mu, sigma) to the device, then the generators from the sweep's own device s-grids
// (hadi_jump_matrix_kernel into the zeroed buffer) and, for a shared matrix, the check of the caller's promise -- on every call,
// also before a replay: the matrices are data, not part of a captured loop.  Matrix q is built on row q of the sweep's s-grids:
// the groups of a Jacobian's batch repeat the caller's rows, so the three sets of an eight-column call (jmp_nmat = 3 n_src, or 3
// of a batch of at least 9 bit-equal rows when the matrices are shared) find their source instance's grid there as well.
int stage_jumps(Ctx *c, const Sweep &w) {
    const SweepDesc &d = w.d;
    const HadiLayout &L = w.r.pl.L;
    hipStream_t s = c->stream;
    int rc;
    if ((rc = stage_to_device(c, c->jmp_a.p, d.jmp_a.data(), d.jmp_a.size() * 8)) ||
        (rc = stage_to_device(c, c->jmp_par.p, d.jmp_musig.data(), d.jmp_musig.size() * 8)))
        return rc;
    const size_t gd = (size_t)d.jmp_nmat * hadi_jump_matrix_doubles(L), ne = (size_t)d.jmp_nmat * (L.m1 + 1) * (L.m1 + 1);
    HIP_TRY(c, hipMemsetAsync(c->jmp_G.p, 0, gd * 8, s));
    HIP_TRY(c, hipMemsetAsync(c->jmp_stat.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(hadi_jump_matrix_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, L, d.jmp_nmat, d.d_vec_s,
                       ptr<double>(c->jmp_par), ptr<double>(c->jmp_G));
    if (d.jmp_shared)
        hipLaunchKernelGGL(hadi_jump_grid_check_kernel, dim3((unsigned)(((size_t)d.n * (L.m1 + 1) + 255) / 256)), dim3(256), 0, s, L.m1 + 1,
                           d.n, d.d_vec_s, ptr<int>(c->jmp_stat));
    return HADI_OK;
}

// Sampled ladder: the lists of all n instances to the device, then the tap records and flag words from the sweep's own device
// grids (hadi_sample_locate_kernel) -- on every call, also before a replay: the taps are data, not part of a captured loop.
// The single price node of the ladder is not used: every instance's entry reads "none".
HadiTap *samp_taps(Ctx *c) { return ptr<HadiTap>(c->samp_tap); }
int *samp_flags(Ctx *c, const SweepDesc &d) { return reinterpret_cast<int *>(samp_taps(c) + (size_t)d.n * d.n_samp); }
int stage_samples(Ctx *c, const Sweep &w) {
    const SweepDesc &d = w.d;
    const size_t ns = (size_t)d.n * d.n_samp;
    std::vector<double> in(2 * ns);
    for (int k = 0; k < d.n; k++) {
        const size_t row = (size_t)(d.samp_rows > 1 ? k % d.n_src : 0) * d.n_samp;
        for (int q = 0; q < d.n_samp; q++) {
            in[(size_t)k * d.n_samp + q] = d.spots[row + q];
            in[ns + (size_t)k * d.n_samp + q] = d.scales ? d.scales[row + q] : 1.0;
        }
    }
    int rc;
    if ((rc = stage_to_device(c, c->samp_in.p, in.data(), in.size() * 8))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->snap_node.p, 0xff, sizeof(int) * (size_t)d.n, c->stream));
    hipLaunchKernelGGL(hadi_sample_locate_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, w.r.pl.L, d.n, d.n_samp,
                       d.d_vec_s, d.d_vec_v, d.d_v0_i, d.V_0, ptr<double>(c->samp_in), ptr<double>(c->samp_in) + ns, samp_taps(c),
                       samp_flags(c, d));
    return HADI_OK;
}

// Parameters and dividend tables to the device, the operator tables (setup), the ladder's price nodes (locate), the packed
// state and, for American sweeps, the payoff and its shape -- which decides w.amp.
int stage_inputs(Ctx *c, Sweep &w) {
    const SweepDesc &d = w.d;
    const HadiRoute &r = w.r;
    const HadiLayout &L = r.pl.L;
    const size_t n = d.n, tot = w.tot, st = w.st;
    hipStream_t s = c->stream;
    int rc;
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if ((rc = stage_to_device(c, c->par8.p, d.par8.data(), 8 * 8 * n))) return rc;
    if ((rc = stage_dividends(c, w))) return rc;
    // identity padding rows of Y must read as zeros in the column pass (the row pass never writes them)
    HIP_TRY(c, hipMemsetAsync(c->Y.p, 0, st, s));

    HadiSetupArgs sa;
    sa.L = L; sa.n_inst = d.n;
    sa.vec_s = d.d_vec_s; sa.vec_v = d.d_vec_v; sa.delta_s = d.d_delta_s; sa.delta_v = d.d_delta_v;
    sa.par = ptr<double>(c->par8);
    sa.r_d = d.r_d; sa.r_f = d.r_f; sa.theta = d.theta;
    sa.scoef = ptr<double>(c->scoef); sa.b2row = ptr<double>(c->b2row); sa.rowc = ptr<double>(c->rowc);
    sa.a2i = ptr<double>(c->a2i); sa.pb = ptr<double>(c->pb); sa.rinv = ptr<double>(c->rinv);
    sa.rwork = ptr<double>(c->rwork); sa.ipar = ptr<HadiInstPar>(c->ipar);
    hipLaunchKernelGGL(hadi_setup_kernel, dim3(d.n), dim3(256), 0, s, sa);
    if (r.ladder) {
        if ((rc = stage_to_device(c, c->snap_steps.p, d.snap_steps, sizeof(int) * d.n_snap))) return rc;
        if (d.n_samp > 0) {
            if ((rc = stage_samples(c, w))) return rc;
        } else {
            hipLaunchKernelGGL(hadi_locate_kernel, dim3((d.n + 63) / 64), dim3(64), 0, s, L, d.n, d.d_vec_s, d.d_vec_v, d.S_0, d.d_v0_i, d.V_0,
                               ptr<int>(c->snap_node), ptr<int>(c->status));
        }
    }

    hipLaunchKernelGGL(hadi_pack_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, d.n, d.n_src, d.d_natU, ptr<double>(c->U));
    if (r.bermudan) {  // the payoff, packed as the state is, and the exercise table
        hipLaunchKernelGGL(hadi_pack_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, d.n, d.n_src,
                           d.d_natU0 ? d.d_natU0 : d.d_natU, ptr<double>(c->U0));
        if ((rc = stage_step_flags(c, d, d.ex, w.ex, c->ex_flag))) return rc;
    }
    if (r.barrier && (rc = stage_barrier(c, w))) return rc;
    if (r.cliquet) {  // the payoff only where some fixing carries a weight (need_u0), packed as the state is
        if (r.need_u0 && !r.bermudan)
            hipLaunchKernelGGL(hadi_pack_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, d.n, d.n_src,
                               d.d_natU0 ? d.d_natU0 : d.d_natU, ptr<double>(c->U0));
        if ((rc = stage_cliquet(c, w))) return rc;
    }
    if (r.jumps && (rc = stage_jumps(c, w))) return rc;
    if (r.american) {
        hipLaunchKernelGGL(hadi_pack_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, d.n, d.n_src,
                           d.d_natU0 ? d.d_natU0 : d.d_natU, ptr<double>(c->U0));
        HIP_TRY(c, hipMemsetAsync(c->LAM.p, 0, st, s));  // lambda_bar <- 0, device_solver.hpp:310-313
        if ((rc = ensure(c, c->pay_mis, sizeof(int) * n))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->pay_mis.p, 0, sizeof(int) * n, s));
        hipLaunchKernelGGL(hadi_payoff_shape_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, d.n, ptr<double>(c->U0), ptr<int>(c->pay_mis));
    }
    // American in the P representation: every payoff of the batch must depend on s only.  One small device-to-host copy per
    // solve decides it.
    w.amp = false;
    if (r.read_payoff_shape) {
        std::vector<int> mis(d.n);
        HIP_TRY(c, hipMemcpyAsync(mis.data(), c->pay_mis.p, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        w.amp = true;
        for (int k = 0; k < d.n; k++) w.amp = w.amp && mis[k] == 0;
    }
    HIP_TRY(c, hipGetLastError());
    if (r.f32) {  // round the packed state to fp32; Y's identity padding rows must read as zeros
        hipLaunchKernelGGL(hadi_narrow_kernel, dim3(grid1d(tot)), dim3(256), 0, s, L, ptr<double>(c->U), ptr<float>(c->Uf), tot);
        HIP_TRY(c, hipMemsetAsync(c->Yf.p, 0, st / 2, s));
    }
    return HADI_OK;
}

// The whole-batch argument blocks of the sweep kernels.
void sweep_args(Ctx *c, Sweep &w) {
    const HadiRoute &r = w.r;
    const HadiPlan &pl = r.pl;
    HadiSweepArgs &a = w.a;
    a.U = ptr<double>(c->U); a.Y = ptr<double>(c->Y);
    if (r.f32) {  // the kernels instantiated for float reinterpret these two
        a.U = reinterpret_cast<double *>(c->Uf.p);
        a.Y = reinterpret_cast<double *>(c->Yf.p);
    }
    a.LAM = r.american ? ptr<double>(c->LAM) : nullptr;
    a.U0 = (r.american || r.need_u0) ? ptr<double>(c->U0) : nullptr;
    a.pay_mis = r.american ? ptr<int>(c->pay_mis) : nullptr;
    a.scoef = ptr<double>(c->scoef); a.b2row = ptr<double>(c->b2row); a.rowc = ptr<double>(c->rowc);
    a.pb = ptr<double>(c->pb); a.rinv = ptr<double>(c->rinv); a.ipar = ptr<HadiInstPar>(c->ipar);
    a.L = pl.L; a.n_inst = w.d.n; a.R = pl.R; a.ntiles = pl.ntiles; a.ctiles = pl.ctiles; a.btpw = pl.btpw; a.bgroups = pl.bgroups;
    a.american = r.american ? 1 : 0; a.pos_m1 = pl.pos_m1;
    a.tile_il = c->t.tile_il;
    a.RS = pl.RS; a.sblocks = pl.sblocks;
    a.err = c->err_dev; a.debug = c->t.debug_fault;
    a.R1 = (r.need_v_r1_c2 || r.need_r1) ? ptr<double>(c->R1) : nullptr;
    a.C2 = r.need_v_r1_c2 ? ptr<double>(c->C2) : nullptr;
    a.rs_tab = r.pair_tab ? ptr<double>(c->rs_tab) : nullptr;
    w.av = a;
    if (r.need_v_r1_c2) w.av.U = ptr<double>(c->V);
}

// ---- one launch for the whole time loop ----------------------------------------------------------------------------------
// The small-grid kernels' second argument block: dividend tables and, for batches of mixed maturities, the dispatch order.
int small_args(Ctx *c, const Sweep &w, HadiSmallArgs &sm) {
    const SweepDesc &d = w.d;
    int rc;
    sm.div_flag = nullptr; sm.div_amounts = nullptr; sm.div_pcts = nullptr; sm.vec_s = d.d_vec_s; sm.Nmax = d.Nmax;
    sm.order = nullptr;
    if (!d.uniform_steps) {  // longest-processing-time-first dispatch order
        std::vector<int> order(d.n);
        for (int k = 0; k < d.n; k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            return d.par8[(size_t)x * 8 + 5] > d.par8[(size_t)y * 8 + 5];
        });
        if ((rc = ensure(c, c->order, sizeof(int) * d.n))) return rc;
        if ((rc = stage_to_device(c, c->order.p, order.data(), sizeof(int) * d.n))) return rc;
        sm.order = ptr<int>(c->order);
    }
    sm.flag_stride = w.div.stride;
    if (w.r.have_div) {
        sm.div_flag = ptr<int>(c->div_flag); sm.div_amounts = ptr<double>(c->div_amt); sm.div_pcts = ptr<double>(c->div_pct);
    }
    if (w.r.bermudan) {
        sm.ex_flag = ptr<int>(c->ex_flag); sm.ex_stride = w.ex.stride;
    }
    if (w.r.barrier) {
        sm.ko_flag = ptr<int>(c->ko_flag); sm.ko_stride = w.mon.stride;
        sm.ko_iab = ptr<int>(c->ko_iab); sm.ko_rebate = ptr<double>(c->ko_rebate);
    }
    if (w.r.cliquet) {
        sm.fix_flag = ptr<int>(c->fix_flag); sm.fix_stride = w.fix.stride; sm.fix_w = w.in.fix_weights ? ptr<double>(c->fix_w) : nullptr;
        sm.fix_iref = ptr<int>(c->fix_iref); sm.fix_mode = ptr<int>(c->fix_mode);
    }
    if (w.r.ladder) {
        sm.snap_steps = ptr<int>(c->snap_steps); sm.n_snap = d.n_snap;
        sm.snap_node = ptr<int>(c->snap_node); sm.snap_out = ptr<double>(c->snap_out);
        if (d.n_samp > 0) {
            sm.taps = samp_taps(c); sm.n_samp = d.n_samp; sm.samp_out = ptr<double>(c->samp_out);
        }
    }
    if (w.r.kind == HADI_ROUTE_SMALL_JUMP) {  // the matrix of an instance: (set of its group) x per + (per > 1 ? source : 0), as hadi_jump_sel_kernel has it
        const int per = d.jmp_nmat / d.jmp_sets;
        std::vector<int> mat(d.n);
        for (int k = 0; k < d.n; k++) mat[k] = (d.jmp_sets > 1 ? hadi_jump_set(k / d.n_src) : 0) * per + (per > 1 ? k % d.n_src : 0);
        if ((rc = stage_to_device(c, c->jmp_mat.p, mat.data(), sizeof(int) * d.n))) return rc;
        sm.jmp_G = ptr<double>(c->jmp_G); sm.jmp_a = ptr<double>(c->jmp_a); sm.jmp_mat = ptr<int>(c->jmp_mat);
        sm.jmp_stride = (long long)hadi_jump_matrix_doubles(w.r.pl.L);
    }
    return HADI_OK;
}

// Small grids: the whole instance fits in LDS (hadi_small_jump_kernel, hadi_small_sch_kernel, hadi_small_kernel, hadi_small_seq_kernel, hadi_small_seq2_kernel).
int run_small(Ctx *c, Sweep &w) {
    const SweepDesc &d = w.d;
    const HadiLayout &L = w.r.pl.L;
    HadiSel sel{nullptr, (unsigned)d.n, 64, 0};
    HadiLoopFn fn;
    if (w.r.kind == HADI_ROUTE_SMALL_JUMP) {
        const int W = w.r.small_waves == 8 ? 8 : 4;
        fn = hadi_small_jump_fn(L.B, W);
        if (!fn) return fail(c, HADI_ERR_INTERNAL, "no small-grid jump kernel for grid %dx%d", d.m1, d.m2);
        sel.block = 64 * W; sel.smem = w.r.pl.smem_small_eu;
    } else if (w.r.kind == HADI_ROUTE_SMALL_SCH) {
        fn = hadi_small_sch_fn(L.B, hadi_route_sch(d.scheme));
        if (!fn) return fail(c, HADI_ERR_INTERNAL, "no small-grid kernel of scheme %d for grid %dx%d", d.scheme, d.m1, d.m2);
        sel.smem = hadi_small_sch_smem(L);
    } else {
        sel = hadi_route_small_sel(w.r, d.n);
        if (!sel.k) return fail(c, HADI_ERR_INTERNAL, "no small-grid kernel for grid %dx%d", d.m1, d.m2);
        fn = sel.k->loop;
    }
    c->last_path = hadi_describe_route(w.r, w.in, false);
    HadiSmallArgs sm;
    const int rc = small_args(c, w, sm);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
    hipLaunchKernelGGL(fn, dim3(sel.grid), dim3(sel.block), sel.smem, c->stream, w.a, sm);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
    return HADI_OK;
}

// Instance-resident launch (hadi_team_kernel), between the same two events.  Any failure of the team protocol is recorded by
// the kernel and checked here; the batch is then packed again and *fell_back sends the caller on to the streaming path.
int run_team(Ctx *c, Sweep &w, bool *fell_back) {
    const SweepDesc &d = w.d;
    const HadiLayout &L = w.r.pl.L;
    hipStream_t s = c->stream;
    const bool have_div = w.r.have_div;
    int rc;
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    if ((rc = ensure(c, c->team, 512 * sizeof(int)))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->team.p, 0, 512 * sizeof(int), s));
    HadiTeamArgs ta;
    ta.form = ptr<int>(c->team); ta.bar = ptr<int>(c->team) + 64; ta.nb = c->cu_count / 8; ta.N = d.Nmax;
    ta.div_flag = have_div ? ptr<int>(c->div_flag) : nullptr; ta.flag_stride = w.div.stride;
    ta.div_amounts = have_div ? ptr<double>(c->div_amt) : nullptr; ta.div_pcts = have_div ? ptr<double>(c->div_pct) : nullptr;
    ta.vec_s = d.d_vec_s;
    ta.stamps = reinterpret_cast<unsigned long long *>(ptr<int>(c->team) + 384);
    const size_t smem = hadi_team_smem(L, have_div);
    if (L.B == 8) hipLaunchKernelGGL((hadi_team_kernel<8>), dim3(c->cu_count), dim3(512), smem, s, w.a, ta);
    else hipLaunchKernelGGL((hadi_team_kernel<4>), dim3(c->cu_count), dim3(512), smem, s, w.a, ta);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    const int deverr = __atomic_exchange_n(c->err_host, 0, __ATOMIC_ACQ_REL);
    if (!deverr) {
        c->last_path = hadi_describe_route(w.r, w.in, w.amp, HADI_TEAM_RAN);
        HIP_TRY(c, hipEventRecord(c->ev[2], s));
        return HADI_OK;
    }
    if (deverr & ~HADI_DEVERR_TEAM) __atomic_fetch_or(c->err_host, deverr & ~HADI_DEVERR_TEAM, __ATOMIC_RELAXED);  // (not ours: keep it for finish_timing)
    c->team_failed = 1;
    // start again from the caller's initial condition on the streaming path
    hipLaunchKernelGGL(hadi_pack_kernel, dim3(grid1d(w.tot)), dim3(256), 0, s, L, d.n, d.n_src, d.d_natU, ptr<double>(c->U));
    HIP_TRY(c, hipMemsetAsync(c->Y.p, 0, w.st, s));
    c->last_path = hadi_describe_route(w.r, w.in, w.amp, HADI_TEAM_FELL_BACK);
    *fell_back = true;
    return HADI_OK;
}

// ---- the time loop over the pass kernels ------------------------------------------------------------------------------------
// The whole-batch arguments narrowed to the sub-batch of `cnt` instances from instance `o` on, with its own launch geometry.
HadiSweepArgs sub_args(const Sweep &w, HadiSweepArgs x, int o, int cnt, const HadiPlan &sp) {
    const HadiPlan &pl = w.r.pl;
    const HadiLayout &L = pl.L;
    x.n_inst = cnt; x.R = sp.R; x.ntiles = sp.ntiles; x.ctiles = sp.ctiles; x.btpw = sp.btpw; x.bgroups = sp.bgroups;
    x.RS = sp.RS; x.sblocks = sp.sblocks;
    const size_t so = (size_t)o * L.inst_stride;
    if (w.r.f32) {
        x.U = reinterpret_cast<double *>(reinterpret_cast<float *>(x.U) + so);
        x.Y = reinterpret_cast<double *>(reinterpret_cast<float *>(x.Y) + so);
    } else {
        x.U += so;
        x.Y += so;
    }
    if (x.LAM) x.LAM += so;
    if (x.U0) x.U0 += so;
    if (x.pay_mis) x.pay_mis += o;
    if (x.R1) x.R1 += so;
    if (x.C2) x.C2 += so;
    if (x.rs_tab) x.rs_tab += (size_t)o * L.nrows * 128;
    x.scoef += (size_t)o * pl.n_scoef; x.b2row += (size_t)o * pl.n_b2row; x.rowc += (size_t)o * pl.n_rowc;
    x.pb += (size_t)o * pl.n_pb; x.rinv += (size_t)o * pl.n_rinv; x.ipar += o;
    return x;
}

// Instances that ride on one staged strip of a SHARED jump matrix: as many as still leave two blocks per CU, at most 8.  With
// per-instance matrices every block has one instance.  (Which instances share a block never changes an instance's result.)
int jump_ipg(const Ctx *c, const SweepDesc &d, const HadiLayout &L, int nsb) {
    if (!d.jmp_shared) return 1;
    return (int)std::max(1ll, std::min(8ll, (long long)nsb * hadi_jump_nib(L) / (2ll * c->cu_count)));
}

// The lists of hadi_jump_sel_kernel for the sub-batch [o, o + nsb) of an eight-column Jacobian's batch.  Shared matrices: runs of
// consecutive instances, as jump_ipg has them (the groups 0 .. 6 are one matrix).  Per-instance matrices: with "jump_share" the set-0
// instances of one source instance ride on one staged strip, up to 7 and by jump_ipg's rule of two blocks per CU; else one
// instance per block.
HadiJumpSel jump_sel(const Ctx *c, const SweepDesc &d, const HadiLayout &L, int o, int nsb) {
    HadiJumpSel q;
    q.inst0 = o; q.n_src = d.n_src; q.per = d.jmp_nmat / d.jmp_sets;
    q.share = (!d.jmp_shared && c->t.jump_share) ? 1 : 0;
    q.cap = q.share ? (int)std::max(1ll, std::min(7ll, (long long)nsb * hadi_jump_nib(L) / (2ll * c->cu_count))) : jump_ipg(c, d, L, nsb);
    return q;
}

// Sub-batch `sb` through its whole time loop on stream q.
int enqueue_sub_batch(Ctx *c, const Sweep &w, int sb, hipStream_t q) {
    const SweepDesc &d = w.d;
    const HadiRoute &r = w.r;
    const HadiLayout &L = r.pl.L;
    const HadiSubBatch &sub = r.bp.subs[sb];
    const HadiPlan &sp = sub.pl;  // launch geometry of THIS sub-batch
    const int o = sub.off, nsb = sub.cnt;
    const bool cs = r.cs, f32 = r.f32, have_div = r.have_div, amp = w.amp;
    const int n_first = d.debug ? d.debug_step : 1, n_last = d.debug ? d.debug_step : d.Nmax;
    const size_t so = (size_t)o * L.inst_stride;
    const HadiSweepArgs a = sub_args(w, w.a, o, nsb, sp), av = sub_args(w, w.av, o, nsb, sp);
    const size_t tot = (size_t)L.inst_stride * nsb, st = tot * sizeof(double);  // the sub-batch's packed state
    double *const Ub = ptr<double>(c->U) + so, *const LAMb = r.american ? ptr<double>(c->LAM) + so : nullptr;
    double *const U0b = (r.american || r.need_u0) ? ptr<double>(c->U0) + so : nullptr, *const UTb = r.need_ut ? ptr<double>(c->UT) + so : nullptr;
    const int ev0 = 4 * sb * d.Nmax;  // profiling events of this sub-batch
    int rc;
    if (r.pair_tab && sp.use_strip) {  // paired strips: the pairs' coupling column, once per solve (hadi_strip_step, RSTAB)
        HadiSweepArgs at = a;
        at.U = Ub;  // (any packed fp64 array: the table depends on the matrix only)
        if ((rc = launch_pass(c, hadi_select_pair_table(sp), q, at, 1))) return rc;
    }
    if (r.resident[sb])  // the sub-batch's whole time loop in one launch (LDS: the strip rings; the column phase aliases them)
        return launch_pass(c, hadi_select_resident(sp), q, a, n_last);
    for (int nstep = n_first; nstep <= n_last; nstep++) {
        // P representation: the first step (the caller's initial U need not dominate the payoff) and dividend steps
        // (the jump acts on U alone) run on the explicit (U, lambda_bar) pair, converted on the way in and out
        const bool xstep = amp && (nstep == 1 || (have_div && w.div.any[nstep]));
        if (xstep && nstep > 1)
            hipLaunchKernelGGL(hadi_am_materialise_kernel, dim3(grid1d(tot)), dim3(256), 0, q, L, nsb, a.ipar, U0b, Ub, LAMb, sp.pos_m1);
        if (have_div && w.div.any[nstep]) {  // device_solver.hpp:426-517: U_temp <- U, U <- interpolated jump
            if (f32)  // fp32 state: the jump works on the fp64 packed array -- widen, jump, round again (<= num_dividends steps)
                hipLaunchKernelGGL(hadi_widen_kernel, dim3(grid1d(tot)), dim3(256), 0, q, L, reinterpret_cast<const float *>(a.U), Ub, tot);
            HIP_TRY(c, hipMemcpyAsync(UTb, Ub, st, hipMemcpyDeviceToDevice, q));
            const size_t npts = (size_t)nsb * L.nrows * (L.m1 + 1);
            hipLaunchKernelGGL(hadi_dividend_kernel, dim3(grid1d(npts)), dim3(256), 0, q, L, nsb, a.ipar,
                               d.d_vec_s + (size_t)o * (L.m1 + 1), UTb, Ub, ptr<int>(c->div_flag) + (size_t)o * w.div.stride,
                               w.div.stride, nstep, ptr<double>(c->div_amt), ptr<double>(c->div_pct));
            if (f32)
                hipLaunchKernelGGL(hadi_narrow_kernel, dim3(grid1d(tot)), dim3(256), 0, q, L, Ub, reinterpret_cast<float *>(a.U), tot);
        }
        hipEvent_t *const kev = r.prof ? &c->kev[ev0 + 4 * (nstep - 1)] : nullptr;
        if (kev) HIP_TRY(c, hipEventRecord(kev[0], q));
        const HadiPassCtx pc{sp, nsb, r.american, amp, xstep, f32, d.scheme, c->t.cs_strips, c->t.col_prefetch};
        const HadiSel col = hadi_select_col_pass(pc);
        if (d.debug == 2) {  // diagnostics: one column solve of the packed input (moved to Y), nothing else
            HIP_TRY(c, hipMemcpyAsync(a.Y, a.U, f32 ? st / 2 : st, hipMemcpyDeviceToDevice, q));
            if ((rc = launch_pass(c, col, q, a, nstep))) return rc;
            break;
        }
        if ((rc = launch_pass(c, hadi_select_row_pass(pc, cs ? 1 : 0), q, a, nstep))) return rc;
        if (d.debug == 1) break;  // diagnostics: Y now holds the right-hand side of the A2 solve
        if (kev) {
            HIP_TRY(c, hipEventRecord(kev[1], q));
            HIP_TRY(c, hipEventRecord(kev[2], q));
        }
        if ((rc = launch_pass(c, col, q, cs ? av : a, nstep))) return rc;
        if (kev) HIP_TRY(c, hipEventRecord(kev[3], q));
        if (cs) {  // corrector (profiling events cover the predictor's two passes only)
            if ((rc = launch_pass(c, hadi_select_row_pass(pc, 2), q, av, nstep)) || (rc = launch_pass(c, col, q, a, nstep))) return rc;
        }
        if (r.jumps) {  // Bates: U_temp <- U, U <- U_temp + a G U_temp behind the step's last column pass, in front of the step's events
            HIP_TRY(c, hipMemcpyAsync(UTb, Ub, st, hipMemcpyDeviceToDevice, q));
            if (d.jmp_sets > 1) {  // the nine groups of an eight-column Jacobian: three matrix sets, picked by group
                const HadiJumpSel js = jump_sel(c, d, L, o, nsb);
                hipLaunchKernelGGL(hadi_jump_sel_kernel, dim3(hadi_jump_sel_grid(L, js, nsb)), dim3(HADI_JUMP_THREADS), hadi_jump_smem(L), q, L,
                                   nsb, js, UTb, Ub, ptr<double>(c->jmp_G), (long long)hadi_jump_matrix_doubles(L), ptr<double>(c->jmp_a) + o,
                                   a.ipar, nstep);
            } else {
                const int ipg = jump_ipg(c, d, L, nsb);
                hipLaunchKernelGGL(hadi_jump_kernel, dim3(hadi_jump_grid(L, nsb, ipg)), dim3(HADI_JUMP_THREADS), hadi_jump_smem(L), q, L, nsb,
                                   ipg, o, d.n_src, UTb, Ub, ptr<double>(c->jmp_G), d.jmp_shared ? 0ll : (long long)hadi_jump_matrix_doubles(L),
                                   ptr<double>(c->jmp_a) + o, a.ipar, nstep);
            }
        }
        if (r.bermudan && w.ex.any[nstep]) {  // Bermudan exercise behind the step's last column pass (European sweeps: U is explicit)
            const int bpi = hadi_exercise_bpi(L);
            hipLaunchKernelGGL(hadi_exercise_kernel, dim3((unsigned)nsb * bpi), dim3(HADI_EX_THREADS), 0, q, L, nsb, bpi, Ub, U0b,
                               ptr<int>(c->ex_flag) + (size_t)o * w.ex.stride, w.ex.stride, nstep);
        }
        if (r.barrier && w.mon.any[nstep]) {  // knock-out behind the step's last column pass (European sweeps, fp64 state: U is explicit)
            const int bpi = hadi_exercise_bpi(L);
            hipLaunchKernelGGL(hadi_knockout_kernel, dim3((unsigned)nsb * bpi), dim3(HADI_EX_THREADS), 0, q, L, nsb, bpi, Ub,
                               ptr<int>(c->ko_flag) + (size_t)o * w.mon.stride, w.mon.stride, ptr<int>(c->ko_iab) + 2 * (size_t)o,
                               ptr<double>(c->ko_rebate) + o, nstep);
        }
        if (r.cliquet && w.fix.any[nstep]) {  // strike fixing behind the step's last column pass: the reference values out, then the event
            const int bpi = hadi_exercise_bpi(L), c_stride = L.nrows_pad;
            const int *const ff = ptr<int>(c->fix_flag) + (size_t)o * w.fix.stride, *const ir = ptr<int>(c->fix_iref) + o;
            double *const cb = ptr<double>(c->fix_c) + (size_t)o * c_stride;
            hipLaunchKernelGGL(hadi_fixing_gather_kernel, dim3((unsigned)(((size_t)nsb * L.nrows + 255) / 256)), dim3(256), 0, q, L, nsb, Ub, ff,
                               w.fix.stride, ir, cb, c_stride, nstep);
            hipLaunchKernelGGL(hadi_fixing_kernel, dim3((unsigned)nsb * bpi), dim3(HADI_EX_THREADS), 0, q, L, nsb, bpi, Ub, U0b, ff,
                               w.in.fix_weights ? ptr<double>(c->fix_w) + (size_t)o * w.fix.stride : nullptr, w.fix.stride, ir,
                               ptr<int>(c->fix_mode) + o, cb, c_stride, d.d_vec_s + (size_t)o * (L.m1 + 1), nstep);
        }
        if (r.ladder && w.snap_q[nstep] >= 0 && d.n_samp > 0) {  // a sample call: n_samp interpolants where the ladder copies one node
            const size_t ns = (size_t)nsb * d.n_samp;
            hipLaunchKernelGGL(hadi_sample_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, q, L, nsb, Ub,
                               samp_taps(c) + (size_t)o * d.n_samp, ptr<double>(c->samp_out) + (size_t)o * d.n_snap * d.n_samp, d.n_snap,
                               d.n_samp, w.snap_q[nstep]);
        } else if (r.ladder && w.snap_q[nstep] >= 0)  // (U is explicit here: a ladder call never runs in the P representation)
            hipLaunchKernelGGL(hadi_snap_kernel, dim3((nsb + 63) / 64), dim3(64), 0, q, L, nsb, Ub, ptr<int>(c->snap_node) + o,
                               ptr<double>(c->snap_out) + (size_t)o * d.n_snap, d.n_snap, w.snap_q[nstep]);
        if (xstep)
            hipLaunchKernelGGL(hadi_am_dematerialise_kernel, dim3(grid1d(tot)), dim3(256), 0, q, L, nsb, a.ipar, U0b, Ub, LAMb);
    }
    if (amp)  // explicit U and lambda_bar for the outputs
        hipLaunchKernelGGL(hadi_am_materialise_kernel, dim3(grid1d(tot)), dim3(256), 0, q, L, nsb, a.ipar, U0b, Ub, LAMb, sp.pos_m1);
    return HADI_OK;
}

// The whole time loop as a function of the stream, so it can be enqueued directly or captured: one sub-batch after the other
// (per stream), each through its whole time loop.
int enqueue_body(Ctx *c, const Sweep &w, hipStream_t q0, bool *forked) {
    const HadiBatchPlan &bp = w.r.bp;
    for (int sb = 0; sb < (int)bp.subs.size(); sb++) {
        if (bp.two_streams && sb == bp.fork_before) {  // fork: the second stream starts behind everything enqueued so far
            HIP_TRY(c, hipEventRecord(c->fork_ev, q0));
            HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->fork_ev, 0));
            *forked = true;
        }
        const int rc = enqueue_sub_batch(c, w, sb, (bp.two_streams && bp.subs[sb].lane) ? c->stream2 : q0);
        if (rc) return rc;
    }
    return HADI_OK;
}
// Fork / join around the body.  The join is enqueued even when the body failed half way: a second stream left un-joined
// would make hipStreamEndCapture fail ("unjoined work") and stay in capture mode for the handle's next call.
int enqueue_loop(Ctx *c, const Sweep &w, hipStream_t q0) {
    bool forked = false;
    const int rcb = enqueue_body(c, w, q0, &forked);
    if (forked) {  // join
        const hipError_t e1 = hipEventRecord(c->join_ev, c->stream2);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(q0, c->join_ev, 0) : e1;
        if (!rcb && e2 != hipSuccess) return fail(c, HADI_ERR_HIP, "joining the second stream failed: %s", hipGetErrorString(e2));
    }
    return rcb;
}

// Every kernel argument is baked into the nodes of a captured loop, so the key is everything they depend on.  Addresses: every
// pointer of both argument blocks, and every array enqueue_sub_batch names itself (the fp64 packed U, which the table kernel and
// the fp32 dividend steps use even when the state is fp32; lambda_bar, payoff, U_temp, the dividend tables and the caller's
// s-grid).  The library's buffers only move when ensure() grows one, and that empties the cache (drop_graphs).
std::string graph_key(const Ctx *c, const Sweep &w) {
    const SweepDesc &d = w.d;
    const HadiSweepArgs &a = w.a;
    const HadiPlan &pl = w.r.pl;
    const HadiBatchPlan &bp = w.r.bp;
    std::string key;
    auto put = [&](const void *p_, size_t nbytes) { key.append(static_cast<const char *>(p_), nbytes); };
    {  // field by field: struct padding is not initialised
        const void *pa[HADI_SWEEP_ARGS_NPTRS], *pv[HADI_SWEEP_ARGS_NPTRS];
        hadi_sweep_args_ptrs(a, pa);
        hadi_sweep_args_ptrs(w.av, pv);
        const void *own[] = {c->U.p, c->LAM.p, c->U0.p, c->UT.p, c->div_flag.p, c->div_amt.p, c->div_pct.p, d.d_vec_s};
        const int ints[] = {a.debug, a.L.m1, a.L.m2, a.L.B, a.L.G, a.L.P, a.n_inst, a.R, a.ntiles, a.ctiles, a.btpw, a.bgroups,
                            a.american, a.pos_m1, d.scheme, d.prec, (int)w.amp, (int)bp.two_streams, (int)bp.subs.size(), pl.row_seq, pl.col_seq, pl.use_pairs, pl.use_strip, pl.RS, pl.sblocks, pl.grid_as, pl.grid_a, pl.grid_b, pl.block_b, pl.W, (int)pl.smem_a, (int)pl.smem_b};
        put(pa, sizeof(pa));
        put(pv, sizeof(pv));
        put(own, sizeof(own));
        put(ints, sizeof(ints));
    }
    for (size_t sb = 0; sb < bp.subs.size(); sb++) {  // the launch geometry of EVERY sub-batch is baked into the nodes (unequal halves
                                                      // on two streams, a tuning change that flips only the second sub-batch's plan)
        const HadiSubBatch &sbt = bp.subs[sb];
        const HadiPlan &q = sbt.pl;
        const int geo[] = {c->t.col_prefetch, c->t.cs_strips, c->t.tile_il, sbt.lane, bp.fork_before, sbt.off, sbt.cnt, q.R, q.ntiles, q.grid_a, (int)q.smem_a, q.use_strip, q.use_pairs, q.RS, q.sblocks, q.grid_as,
                           (int)q.smem_as, q.ctiles, q.btpw, q.bgroups, q.grid_b, q.block_b, (int)q.smem_b, q.row_seq, q.col_seq, q.W, q.NG, q.PD,
                           w.r.resident[sb] ? 1 : 0};
        put(geo, sizeof(geo));
    }
    put(&d.Nmax, sizeof(int)); put(&d.dt0, sizeof(double));
    put(&d.variant, sizeof(int));
    if (w.r.ladder) {  // the snapshot launches sit behind the steps of the list, with these addresses
        const void *lad[] = {c->snap_node.p, c->snap_out.p};
        put(lad, sizeof(lad));
        put(&d.n_snap, sizeof(int));
        put(d.snap_steps, sizeof(int) * d.n_snap);
        const void *smp[] = {c->samp_tap.p, c->samp_out.p};  // a sample call: hadi_sample_kernel in hadi_snap_kernel's place
        put(&d.n_samp, sizeof(int));
        if (d.n_samp > 0) put(smp, sizeof(smp));
    }
    // A step table (dividends, exercise, monitoring) is re-uploaded every call; the node list only depends on the table's address,
    // on its stride and on which steps carry the table's launch -- the three items this puts.  (The dividend table's address is
    // among `own` above as well: it stands in the key twice.)
    auto put_table = [&](const DevBuf &table, const StepTable &t) {
        put(&table.p, sizeof(void *));
        put(&t.stride, sizeof(int));
        put(t.any.data(), t.any.size());
    };
    if (w.r.bermudan) put_table(c->ex_flag, w.ex);  // (the payoff's address is in both argument blocks)
    if (w.r.barrier) {  // the index ranges are located again every call; the knock-out launches name them and the rebates
        const void *ko[] = {c->ko_iab.p, c->ko_rebate.p};
        put(ko, sizeof(ko));
        put_table(c->ko_flag, w.mon);
    }
    if (w.r.cliquet) {  // the nodes are located again every call; the launches name them, the weights, the modes and c
        const void *fx[] = {c->fix_iref.p, c->fix_mode.p, c->fix_c.p, w.in.fix_weights ? c->fix_w.p : nullptr};
        put(fx, sizeof(fx));
        put_table(c->fix_flag, w.fix);
    }
    if (w.r.jumps) {  // the matrices and the weights are built again every call; the launches name their addresses (U_temp: `own`
                      // above), the matrix stride (0: shared), the source count and the instances per block
        const void *jm[] = {c->jmp_G.p, c->jmp_a.p};
        const int ji[] = {(int)d.jmp_shared, d.n_src, c->cu_count, d.jmp_sets, c->t.jump_share};
        put(jm, sizeof(jm));
        put(ji, sizeof(ji));
    }
    if (w.r.have_div) put_table(c->div_flag, w.div);  // (amounts / percentages: `own` above)
    return key;
}

// Replays the time loop from the graph cached under `key`, capturing it first (and evicting the least recently used of 8
// entries) when there is none.
int replay_or_capture(Ctx *c, const Sweep &w, const std::string &key) {
    hipStream_t s = c->stream;
    Ctx::GraphEntry *hit = nullptr;
    for (auto &g : c->graphs)
        if (g.key == key) { hit = &g; break; }
    if (!hit) {
        if (c->graphs.size() >= 8) {  // evict the least recently used entry
            size_t lru = 0;
            for (size_t k = 1; k < c->graphs.size(); k++)
                if (c->graphs[k].stamp < c->graphs[lru].stamp) lru = k;
            (void)hipGraphExecDestroy(c->graphs[lru].exec);
            (void)hipGraphDestroy(c->graphs[lru].graph);
            c->graphs.erase(c->graphs.begin() + lru);
            c->graph_evictions++;
        }
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_TRY(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rcl = enqueue_loop(c, w, s);
        hipError_t ec = hipStreamEndCapture(s, &graph);
        if (rcl || ec != hipSuccess) {  // nothing half-built survives: the captured graph is dropped
            if (graph) (void)hipGraphDestroy(graph);
            if (rcl) return rcl;
        }
        HIP_TRY(c, ec);
        HIP_TRY(c, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        c->graphs.push_back(Ctx::GraphEntry{key, graph, exec, 0});
        hit = &c->graphs.back();
        c->graph_captures++;
    } else {
        c->graph_replays++;
    }
    hit->stamp = ++c->graph_clock;
    HIP_TRY(c, hipGraphLaunch(hit->exec, s));
    return HADI_OK;
}

int run_streaming(Ctx *c, Sweep &w, bool team_fell_back) {
    hipStream_t s = c->stream;
    int rc;
    if (!team_fell_back) {  // (the team's attempt has set both)
        c->last_path = hadi_describe_route(w.r, w.in, w.amp);
        HIP_TRY(c, hipEventRecord(c->ev[1], s));
    }
    if ((rc = w.r.graphable ? replay_or_capture(c, w, graph_key(c, w)) : enqueue_loop(c, w, s))) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (w.r.f32)  // back to the fp64 packed array the unpack / price-pick kernels read
        hipLaunchKernelGGL(hadi_widen_kernel, dim3(grid1d(w.tot)), dim3(256), 0, s, w.r.pl.L, ptr<float>(c->Uf), ptr<double>(c->U), w.tot);
    return HADI_OK;
}

int run_sweep(Ctx *c, const SweepDesc &d, HadiPlan &pl) {
    Sweep w{d, route_in(c, d)};
    w.in.n_ex_steps = mark_steps(d, d.ex, w.ex);
    w.in.n_mon_steps = mark_steps(d, d.mon, w.mon);
    w.in.n_fix_steps = mark_steps(d, d.fix, w.fix);
    for (size_t e = 0; d.fix_weights && e < (size_t)d.fix.rows * d.fix.n_ex; e++)
        if (d.fix.steps[e] > 0 && d.fix_weights[e] != 0.0) w.in.fix_weights = true;
    w.r = hadi_route(w.in);
    if (w.r.status == HADI_ROUTE_BAD_GRID)
        return fail(c, HADI_ERR_UNSUPPORTED, "grid %dx%d not supported (need m1 >= 2, m2 >= 3 and (m1 + 16)(m2 + 1) < 2^28)", d.m1, d.m2);
    if (w.r.status == HADI_ROUTE_SEQ_UNSUPPORTED)
        return fail(c, HADI_ERR_UNSUPPORTED, "grids with m1 > 1024 or m2 > %d run Douglas sweeps with the fp64 state only", HADI_MAX_P * HADI_LC - 1);
    if (w.r.status) return fail(c, HADI_ERR_UNSUPPORTED, "plan failed");
    if (w.r.jumps && w.r.seq_shape)
        return fail(c, HADI_ERR_UNSUPPORTED, "jump sweeps run the streaming kernels: grids with m1 > 1024 or m2 > %d take the sequential passes", HADI_MAX_P * HADI_LC - 1);
    pl = w.r.pl;
    w.tot = (size_t)pl.L.inst_stride * d.n;
    w.st = w.tot * sizeof(double);
    int rc;
    if ((rc = grow_buffers(c, w)) || (rc = stage_inputs(c, w))) return rc;
    sweep_args(c, w);
    if (w.r.prof) {
        const size_t need = (size_t)4 * d.Nmax * w.r.bp.subs.size();
        while (c->kev.size() < need) {
            hipEvent_t e;
            HIP_TRY(c, hipEventCreate(&e));
            c->kev.push_back(e);
        }
    }
    if (w.r.kind != HADI_ROUTE_TEAM && w.r.kind != HADI_ROUTE_STREAMING) return run_small(c, w);
    c->last_nsub = (int)w.r.bp.subs.size();
    bool fell_back = false;
    if (w.r.kind == HADI_ROUTE_TEAM) {
        c->last_path = hadi_describe_route(w.r, w.in, w.amp);
        if ((rc = run_team(c, w, &fell_back)) || !fell_back) return rc;
    }
    return run_streaming(c, w, fell_back);
}

int finish_timing(Ctx *c, const SweepDesc &d) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->pin_dirty = 0;
    // the sticky device error word (see Ctx::err_host): whatever a kernel of this call reported is visible now
    const int deverr = __atomic_exchange_n(c->err_host, 0, __ATOMIC_ACQ_REL);
    float ms = 0;
    hadi_timing &t = c->timing;
    t = hadi_timing{};
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); t.setup_ms = ms;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); t.sweep_ms = ms;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); t.finish_ms = ms;
    long long ps = 0;
    const long long m = (long long)(d.m1 + 1) * (d.m2 + 1);
    for (int k = 0; k < d.n; k++) ps += m * (long long)d.par8[(size_t)k * 8 + 5];
    t.point_steps = ps;
    if (c->profiling && !d.debug && (int)c->kev.size() >= 4 * d.Nmax * c->last_nsub) {
        for (int k = 0; k < d.Nmax * c->last_nsub; k++) {
            HIP_TRY(c, hipEventElapsedTime(&ms, c->kev[4 * k], c->kev[4 * k + 1])); t.pass_a_ms += ms;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->kev[4 * k + 2], c->kev[4 * k + 3])); t.pass_b_ms += ms;
        }
        t.pass_a_launches = (long long)d.Nmax * c->last_nsub;
        t.pass_b_launches = (long long)d.Nmax * c->last_nsub;
    }
    if (deverr)
        return fail(c, HADI_ERR_INTERNAL, "device-side failure 0x%x during the sweep%s: the results of this call are invalid", deverr,
                    (deverr & HADI_DEVERR_RENDEZVOUS) ? " (a pair rendezvous of a two-wavefront row ran out of polls)" : "");
    return HADI_OK;
}

// Brings an array argument to the device (staging host memory into `buf`).
int to_device(Ctx *c, int memspace, const double *src, size_t count, DevBuf &buf, const double **out) {
    if (!src) { *out = nullptr; return HADI_OK; }
    if (memspace == HADI_MEM_DEVICE) { *out = src; return HADI_OK; }
    int rc = ensure(c, buf, count * sizeof(double));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(buf.p, src, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    *out = ptr<double>(buf);
    return HADI_OK;
}

int from_device(Ctx *c, int memspace, double *dst, const double *dsrc, size_t count) {
    HIP_TRY(c, hipMemcpyAsync(dst, dsrc, count * sizeof(double),
                              memspace == HADI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                              c->stream));
    return HADI_OK;
}

int check_problem(Ctx *c, const hadi_problem *p, bool need_U, bool need_vgrid) {
    if (!c) return HADI_ERR_INVALID;
    if (!p) return fail(c, HADI_ERR_INVALID, "problem is NULL");
    if (p->n_instances < 1) return fail(c, HADI_ERR_INVALID, "n_instances must be >= 1");
    if (p->variant < HADI_EU || p->variant > HADI_AM_DIV) return fail(c, HADI_ERR_INVALID, "bad variant %d", p->variant);
    if (p->memspace != HADI_MEM_HOST && p->memspace != HADI_MEM_DEVICE)
        return fail(c, HADI_ERR_INVALID, "bad memspace %d", p->memspace);
    if (!p->vec_s || !p->delta_s) return fail(c, HADI_ERR_INVALID, "vec_s / delta_s missing");
    if (need_vgrid && (!p->vec_v || !p->delta_v)) return fail(c, HADI_ERR_INVALID, "vec_v / delta_v missing");
    if (need_U && !p->U) return fail(c, HADI_ERR_INVALID, "U missing");
    if (!p->N_i && p->N < 1) return fail(c, HADI_ERR_INVALID, "N must be >= 1");
    if (!p->delta_t_i && !(p->delta_t > 0 && std::isfinite(p->delta_t))) return fail(c, HADI_ERR_INVALID, "delta_t must be > 0");
    for (int k = 0; k < p->n_instances; k++) {  // per-instance overrides: every entry, not only the shared scalars
        if (p->N_i && p->N_i[k] < 1) return fail(c, HADI_ERR_INVALID, "N_i[%d] = %d must be >= 1", k, p->N_i[k]);
        if (p->delta_t_i && !(p->delta_t_i[k] > 0 && std::isfinite(p->delta_t_i[k])))
            return fail(c, HADI_ERR_INVALID, "delta_t_i[%d] = %g must be > 0 and finite", k, p->delta_t_i[k]);
    }
    if (!(p->theta >= 0 && std::isfinite(p->theta))) return fail(c, HADI_ERR_INVALID, "theta must be >= 0");
    if (p->option_type != HADI_CALL && p->option_type != HADI_PUT) return fail(c, HADI_ERR_INVALID, "bad option_type %d", p->option_type);
    if (p->option_type == HADI_PUT) {
        if (!p->strike_i) return fail(c, HADI_ERR_INVALID, "option_type = HADI_PUT needs strike_i (boundary value K e^{-r_d t})");
        for (int k = 0; k < p->n_instances; k++)
            if (!(p->strike_i[k] > 0 && std::isfinite(p->strike_i[k]))) return fail(c, HADI_ERR_INVALID, "strike_i[%d] must be > 0", k);
        if (p->scheme != HADI_SCHEME_DOUGLAS) return fail(c, HADI_ERR_UNSUPPORTED, "put boundary data are available for Douglas steps only");
    }
    if (p->V_0_i && need_vgrid) return fail(c, HADI_ERR_INVALID, "V_0_i applies to hadi_compute_base_prices* / hadi_compute_jacobian* only");
    {  // grid shape, before anything is staged
        HadiPlan tmp;
        if (p->m1 < 2 || p->m2 < 3 ||
            hadi_make_plan(p->m1, p->m2, p->n_instances, 8 * c->cu_count, &tmp, c->t.tune, p->state_precision == HADI_STATE_FP32 ? 4 : 8))
            return fail(c, HADI_ERR_UNSUPPORTED, "grid %dx%d not supported (need m1 >= 2, m2 >= 3 and (m1 + 16)(m2 + 1) < 2^28)", p->m1, p->m2);
    }
    const bool dividend = p->variant == HADI_DIV || p->variant == HADI_AM_DIV;
    if (dividend && p->num_dividends > 0 && (!p->dividend_dates || !p->dividend_amounts || !p->dividend_percentages))
        return fail(c, HADI_ERR_INVALID, "dividend arrays missing");
    if (p->num_dividends < 0) return fail(c, HADI_ERR_INVALID, "num_dividends < 0");
    if (p->scheme != HADI_SCHEME_DOUGLAS && p->scheme != HADI_SCHEME_CRAIG_SNEYD && p->scheme != HADI_SCHEME_MCS && p->scheme != HADI_SCHEME_HV)
        return fail(c, HADI_ERR_INVALID, "bad scheme %d", p->scheme);
    if (p->scheme != HADI_SCHEME_DOUGLAS && p->variant != HADI_EU)
        return fail(c, HADI_ERR_UNSUPPORTED, "the predictor-corrector schemes (Craig-Sneyd, MCS, HV) are available for the European variant only");
    if ((p->scheme == HADI_SCHEME_MCS || p->scheme == HADI_SCHEME_HV) && !(p->theta > 0))
        return fail(c, HADI_ERR_UNSUPPORTED, "MCS / HV steps need theta > 0");
    if (p->state_precision != HADI_STATE_FP64 && p->state_precision != HADI_STATE_FP32)
        return fail(c, HADI_ERR_INVALID, "bad state_precision %d", p->state_precision);
    if (p->state_precision == HADI_STATE_FP32 &&
        ((p->variant != HADI_EU && p->variant != HADI_DIV) || p->scheme != HADI_SCHEME_DOUGLAS))
        return fail(c, HADI_ERR_UNSUPPORTED, "the fp32-state sweep covers European Douglas steps (with or without dividends) only");
    return HADI_OK;
}

// What the ladder entry points ask beyond check_problem (which has passed).  The definition -- snapshot q is what the same call
// with N = snap_steps[q] returns -- needs every table of the sweep to be independent of N.  One is not: the call's boundary
// vector carries exp(-r_f dt (N - 1)) (hes_boundary_kernels.hpp:56, mirrored by hadi_setup_instance), so with call data and
// r_f != 0 the state after n steps of an N-step sweep is NOT the n-step solve, and the ladder refuses such a problem.
int check_ladder(Ctx *c, const hadi_problem *p, int n_snap, const int *snap_steps, const void *out) {
    if (!out) return fail(c, HADI_ERR_INVALID, "ladder output missing");
    if (p->N_i) return fail(c, HADI_ERR_INVALID, "a maturity ladder shares the step indices: N_i must be NULL (delta_t_i is allowed)");
    if (!snap_steps || n_snap < 1 || n_snap > p->N) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    for (int q = 0; q < n_snap; q++)
        if (snap_steps[q] < 1 || snap_steps[q] > p->N || (q && snap_steps[q] <= snap_steps[q - 1]))
            return fail(c, HADI_ERR_INVALID, "snap_steps must be strictly increasing within 1..N (entry %d is %d)", q, snap_steps[q]);
    if (p->state_precision == HADI_STATE_FP32) return fail(c, HADI_ERR_UNSUPPORTED, "the maturity ladder needs the fp64 state");
    if (p->option_type == HADI_CALL && p->r_f != 0.0)
        return fail(c, HADI_ERR_UNSUPPORTED, "call boundary data carry exp(-r_f dt (N - 1)): with r_f != 0 the intermediate states of a "
                                             "sweep are not the shorter sweeps' results, so there is no ladder");
    return HADI_OK;
}

// What the sample entry points ask beyond check_ladder (which has passed): they are refused exactly where the ladder is.
int check_samples(Ctx *c, const hadi_problem *p, const hadi_samples *sp) {
    if (!sp || !sp->spots) return fail(c, HADI_ERR_INVALID, "samples (struct or spots) missing");
    if (sp->n_samp < 1 || sp->n_samp > 1024) return fail(c, HADI_ERR_INVALID, "n_samp must be within 1..1024 (is %d)", sp->n_samp);
    if (sp->rows != 1 && sp->rows != p->n_instances) return fail(c, HADI_ERR_INVALID, "samples: rows must be 1 or n_instances");
    if (sp->scales)
        for (size_t e = 0; e < (size_t)sp->rows * sp->n_samp; e++)
            if (!std::isfinite(sp->scales[e])) return fail(c, HADI_ERR_INVALID, "samples: scale %zu is not finite", e);
    return HADI_OK;
}
// After the sweep of a sample call: the samples' flag words decide the status (they came back with the stream synchronisation).
int samples_status(Ctx *c, const int *flags, size_t count, int n_samp) {
    for (size_t e = 0; e < count; e++)
        if (flags[e] & HADI_SAMPLE_DEGENERATE)
            return fail(c, HADI_ERR_INVALID, "sample %zu of instance %zu: degenerate stencil (an s-interval of length zero, or m1 < 3)", e % n_samp, e / n_samp);
    for (size_t e = 0; e < count; e++)
        if (flags[e]) return fail(c, HADI_ERR_NOT_ON_GRID, "sample %zu of instance %zu is off the s-grid", e % n_samp, e / n_samp);
    return HADI_OK;
}

// What the Bermudan entry points ask beyond check_problem (which has passed).
int check_bermudan(Ctx *c, const hadi_problem *p, const ExSched &ex) {
    if (p->variant == HADI_AM || p->variant == HADI_AM_DIV)
        return fail(c, HADI_ERR_UNSUPPORTED, "a Bermudan sweep is the European sweep (HADI_EU or HADI_DIV) with exercise steps");
    if (p->state_precision == HADI_STATE_FP32) return fail(c, HADI_ERR_UNSUPPORTED, "Bermudan sweeps need the fp64 state");
    if (ex.n_ex < 0) return fail(c, HADI_ERR_INVALID, "n_ex must be >= 0");
    if (ex.rows != 1 && ex.rows != p->n_instances) return fail(c, HADI_ERR_INVALID, "ex_rows must be 1 or n_instances");
    if (ex.n_ex > 0 && !ex.steps) return fail(c, HADI_ERR_INVALID, "ex_steps missing");
    for (int k = 0; k < ex.rows; k++) {
        int Nk = p->N_i ? p->N_i[k] : p->N;
        if (ex.rows == 1 && p->N_i)  // one schedule for the batch: within every instance's time loop
            for (int z = 0; z < p->n_instances; z++) Nk = std::min(Nk, p->N_i[z]);
        const int *row = ex.steps + (size_t)k * ex.n_ex;
        for (int q = 0; q < ex.n_ex; q++) {
            if (row[q] == 0) {
                for (int z = q + 1; z < ex.n_ex; z++)
                    if (row[z] != 0) return fail(c, HADI_ERR_INVALID, "ex_steps row %d: entry %d is non-zero behind a zero", k, z);
                break;
            }
            if (row[q] < 1 || row[q] > Nk || (q && row[q] <= row[q - 1]))
                return fail(c, HADI_ERR_INVALID, "ex_steps row %d must be strictly increasing within 1..%d (entry %d is %d)", k, Nk, q, row[q]);
        }
    }
    return HADI_OK;
}

// What the barrier entry points ask beyond check_problem (which has passed).  The schedule follows the rules of ex_steps.
int check_barrier(Ctx *c, const hadi_problem *p, const hadi_barrier *b) {
    if (p->variant == HADI_AM || p->variant == HADI_AM_DIV)
        return fail(c, HADI_ERR_UNSUPPORTED, "a barrier sweep is the European sweep (HADI_EU or HADI_DIV) with monitoring steps");
    if (p->state_precision == HADI_STATE_FP32) return fail(c, HADI_ERR_UNSUPPORTED, "barrier sweeps need the fp64 state");
    const int n = p->n_instances;
    for (int k = 0; k < n; k++) {
        const double lo = b->lower_i ? b->lower_i[k] : -INFINITY, up = b->upper_i ? b->upper_i[k] : INFINITY;
        if (std::isnan(lo) || std::isnan(up)) return fail(c, HADI_ERR_INVALID, "instance %d: a barrier is NaN", k);
        if (lo >= up) return fail(c, HADI_ERR_INVALID, "instance %d: lower barrier %g is not below the upper barrier %g", k, lo, up);
        if (b->rebate_i && !std::isfinite(b->rebate_i[k])) return fail(c, HADI_ERR_INVALID, "instance %d: the rebate is not finite", k);
    }
    if (b->n_mon > 0 && !b->lower_i && !b->upper_i) return fail(c, HADI_ERR_INVALID, "monitoring steps without a barrier on either side");
    const ExSched mon{b->n_mon, b->mon_rows, b->mon_steps};
    const int rc = check_bermudan(c, p, mon);
    if (rc == HADI_ERR_INVALID) c->err = "mon_steps (the rules of ex_steps): " + c->err;
    return rc;
}

// What the cliquet entry points ask beyond check_problem (which has passed).  The schedule follows the rules of ex_steps.
static_assert(HADI_FIX_SHARES == HADI_FIXM_SHARES && HADI_FIX_RETURN == HADI_FIXM_RETURN, "hadi.h / hadi_k_fixing.h modes");
int check_cliquet(Ctx *c, const hadi_problem *p, const hadi_cliquet *q) {
    if (p->variant == HADI_AM || p->variant == HADI_AM_DIV)
        return fail(c, HADI_ERR_UNSUPPORTED, "a cliquet sweep is the European sweep (HADI_EU or HADI_DIV) with fixing steps");
    if (p->state_precision == HADI_STATE_FP32) return fail(c, HADI_ERR_UNSUPPORTED, "cliquet sweeps need the fp64 state");
    const ExSched fix{q->n_fix, q->fix_rows, q->fix_steps};
    const int rc = check_bermudan(c, p, fix);
    if (rc == HADI_ERR_INVALID) c->err = "fix_steps (the rules of ex_steps): " + c->err;
    if (rc) return rc;
    const int n = p->n_instances;
    if (q->n_fix > 0 && !q->ref_spot_i) return fail(c, HADI_ERR_INVALID, "ref_spot_i missing");
    for (int k = 0; k < n; k++) {
        const int mode = q->mode_i ? q->mode_i[k] : HADI_FIX_SHARES;
        if (mode != HADI_FIX_SHARES && mode != HADI_FIX_RETURN) return fail(c, HADI_ERR_INVALID, "instance %d: fixing mode %d is neither 0 nor 1", k, mode);
        if (!q->ref_spot_i) continue;
        if (!std::isfinite(q->ref_spot_i[k])) return fail(c, HADI_ERR_INVALID, "instance %d: the reference spot is not finite", k);
        if (mode == HADI_FIX_SHARES && q->ref_spot_i[k] <= 1e-10)
            return fail(c, HADI_ERR_INVALID, "instance %d: HADI_FIX_SHARES needs a reference spot above 1e-10 (node 0 is the grid's 0)", k);
    }
    for (size_t e = 0; q->weights && e < (size_t)q->fix_rows * q->n_fix; e++)
        if (q->fix_steps[e] > 0 && !std::isfinite(q->weights[e])) return fail(c, HADI_ERR_INVALID, "weights: entry %zu is not finite", e);
    return HADI_OK;
}

// What the Bates entry points ask beyond check_problem (which has passed).
// bump: what the lambda group of an eight-column Jacobian adds to every intensity (0: no such group).
int check_jumps(Ctx *c, const hadi_problem *p, const hadi_jumps *j, double bump) {
    if (p->variant == HADI_AM || p->variant == HADI_AM_DIV)
        return fail(c, HADI_ERR_UNSUPPORTED, "a jump sweep is the European sweep (HADI_EU or HADI_DIV) with a jump sub-step");
    if (p->state_precision == HADI_STATE_FP32) return fail(c, HADI_ERR_UNSUPPORTED, "jump sweeps need the fp64 state");
    for (int k = 0; k < p->n_instances; k++) {
        const double lam = j->lambda_i ? j->lambda_i[k] : j->lambda, mu = j->mu_i ? j->mu_i[k] : j->mu, sg = j->sigma_i ? j->sigma_i[k] : j->sigma;
        const double dt = p->delta_t_i ? p->delta_t_i[k] : p->delta_t;
        if (!std::isfinite(lam) || !std::isfinite(mu) || !std::isfinite(sg)) return fail(c, HADI_ERR_INVALID, "instance %d: a jump parameter is not finite", k);
        if (lam < 0.0) return fail(c, HADI_ERR_INVALID, "instance %d: jump intensity %g is negative", k, lam);
        if (!(sg > 0.0)) return fail(c, HADI_ERR_INVALID, "instance %d: jump volatility %g is not positive", k, sg);
        if (lam * dt > 1.0)
            return fail(c, HADI_ERR_INVALID, "instance %d: lambda delta_t = %g exceeds 1 (the weight of the identity in the jump sub-step would turn negative)", k, lam * dt);
        if (bump != 0.0 && !((lam + bump) * dt <= 1.0))
            return fail(c, HADI_ERR_INVALID, "instance %d: (lambda + eps) delta_t = %g exceeds 1 in the Jacobian's lambda group", k, (lam + bump) * dt);
    }
    return HADI_OK;
}

// What a call may carry beyond the problem, as its entry point received it.  Every entry point fills the fields of its feature
// by name and leaves the others as they are here.  A new per-call feature goes here, into check_extras and into apply_extras.
struct CallExtras {
    bool ladder = false;  // a ladder or sample entry point: prices after each of snap_steps[0 .. n_snap)
    int n_snap = 0; const int *snap_steps = nullptr;
    bool sampled = false; const hadi_samples *samples = nullptr;  // a sample entry point (NULL is not "absent": check_samples refuses it)
    bool bermudan = false; ExSched ex;                            // a Bermudan entry point, with its exercise schedule
    const hadi_barrier *barrier = nullptr;                        // a barrier entry point (each refuses NULL itself)
    const hadi_cliquet *cliquet = nullptr;                        // a cliquet entry point (each refuses NULL itself)
    const hadi_jumps *jumps = nullptr;                            // a Bates entry point (each refuses NULL itself)
    bool jump_cols = false; double jump_eps = 0;                  // ... whose Jacobian has the columns lambda, mu_J, sigma_J: 9 groups, step eps
    int debug = 0, debug_step = 1; double *debug_out = nullptr;   // diagnostics (hadi_debug_*): SweepDesc::debug, and where the pass's result goes
};

// Where a call's results go and what is picked.
struct CallOut {
    bool rebuild_v = false;  // the v-grids are rebuilt for V_0 (or V_0_i) instead of taken from the caller
    bool pick = false;       // the prices of the node (S_0, V_0) go to `prices`
    double S_0 = 0, V_0 = 0, eps = 0;
    double *prices = nullptr;                      // solve_common: [n], or the ladder's [n][n_snap] / the samples' [n][n_snap][n_samp]
    double *J = nullptr, *base_prices = nullptr;   // jacobian_common
    double *greeks = nullptr, *ladder = nullptr;   // greeks_common
};

// The features' checks behind check_problem (which has passed), in this order.  ladder_out: where a ladder call's output goes.
int check_extras(Ctx *c, const hadi_problem *p, const CallExtras &x, const void *ladder_out) {
    int rc;
    if (x.bermudan && (rc = check_bermudan(c, p, x.ex))) return rc;
    if (x.barrier && (rc = check_barrier(c, p, x.barrier))) return rc;
    if (x.cliquet && (rc = check_cliquet(c, p, x.cliquet))) return rc;
    if (x.jumps && (rc = check_jumps(c, p, x.jumps, x.jump_cols ? x.jump_eps : 0.0))) return rc;
    if (x.ladder && (rc = check_ladder(c, p, x.n_snap, x.snap_steps, ladder_out))) return rc;
    if (x.sampled && (rc = check_samples(c, p, x.samples))) return rc;
    return HADI_OK;
}

// The (checked) extras into the sweep's description.  d_v0_i: the per-instance V_0 of a ladder's price nodes (device, or null).
void apply_extras(SweepDesc &d, const CallExtras &x, const CallOut &o, const double *d_v0_i) {
    d.debug = x.debug; d.debug_step = x.debug_step;
    if (x.ladder) {
        d.n_snap = x.n_snap; d.snap_steps = x.snap_steps; d.S_0 = o.S_0; d.V_0 = o.V_0; d.d_v0_i = d_v0_i;
        if (x.sampled) { d.n_samp = x.samples->n_samp; d.samp_rows = x.samples->rows; d.spots = x.samples->spots; d.scales = x.samples->scales; }
    }
    if (x.bermudan && x.ex.n_ex > 0) d.ex = x.ex;
    if (x.barrier && x.barrier->n_mon > 0) {
        d.mon = ExSched{x.barrier->n_mon, x.barrier->mon_rows, x.barrier->mon_steps};
        d.ko_lower = x.barrier->lower_i; d.ko_upper = x.barrier->upper_i; d.ko_rebate = x.barrier->rebate_i;
    }
    if (x.cliquet && x.cliquet->n_fix > 0) {
        d.fix = ExSched{x.cliquet->n_fix, x.cliquet->fix_rows, x.cliquet->fix_steps};
        d.fix_ref = x.cliquet->ref_spot_i; d.fix_mode = x.cliquet->mode_i; d.fix_weights = x.cliquet->weights;
    }
    if (x.jumps) {  // (fill_desc has run: the rows of par8 hold every instance's delta_t)
        const hadi_jumps &j = *x.jumps;
        std::vector<double> a(d.n);
        bool any = x.jump_cols;  // (the lambda group of an eight-column Jacobian always jumps)
        for (int k = 0; k < d.n; k++) {
            const double lam = j.lambda_i ? j.lambda_i[k % d.n_src] : j.lambda;
            // group 6 of the eight-column Jacobian: lambda + eps.  An instance with lambda = 0 keeps a = 0 in the groups 7 and 8.
            a[k] = ((x.jump_cols && k / d.n_src == 6) ? lam + x.jump_eps : lam) * d.par8[(size_t)k * 8 + 4];
            any = any || a[k] != 0.0;
        }
        if (any) {  // (all weights zero: the plain call, bit for bit, on whatever route it takes)
            d.jmp_a = a;
            d.jmp_shared = j.shared_grid && !j.mu_i && !j.sigma_i;
            d.jmp_sets = x.jump_cols ? HADI_JUMP_SETS : 1;
            const int per = d.jmp_shared ? 1 : d.n_src;
            d.jmp_nmat = d.jmp_sets * per;
            for (int q = 0; q < d.jmp_nmat; q++) {  // set 1: mu + eps, set 2: sigma + eps
                const int set = q / per, k = q % per;
                d.jmp_musig.push_back((j.mu_i ? j.mu_i[k] : j.mu) + (set == 1 ? x.jump_eps : 0.0));
                d.jmp_musig.push_back((j.sigma_i ? j.sigma_i[k] : j.sigma) + (set == 2 ? x.jump_eps : 0.0));
            }
        }
    }
}

// The problem into the sweep's description, as `groups` copies of the caller's batch (a Jacobian: 6) with their parameter rows.
void fill_desc(const hadi_problem *p, SweepDesc &d, int groups) {
    const int n0 = p->n_instances;
    d.n = n0 * groups; d.n_src = n0;
    d.m1 = p->m1; d.m2 = p->m2; d.variant = p->variant; d.scheme = p->scheme; d.prec = p->state_precision;
    d.theta = p->theta; d.r_d = p->r_d; d.r_f = p->r_f;
    const bool dividend = p->variant == HADI_DIV || p->variant == HADI_AM_DIV;
    d.num_div = dividend ? p->num_dividends : 0;
    d.div_dates = p->dividend_dates; d.div_amounts = p->dividend_amounts; d.div_pcts = p->dividend_percentages;
    d.par8.assign((size_t)n0 * groups * 8, 0.0);
    d.Nmax = 0;
    d.uniform_steps = !(p->N_i || p->delta_t_i);
    d.dt0 = p->delta_t;
    for (int g = 0; g < groups; g++)
        for (int k = 0; k < n0; k++) {
            double *r = &d.par8[((size_t)g * n0 + k) * 8];
            r[0] = p->rho_i ? p->rho_i[k] : p->rho;
            r[1] = p->sigma_i ? p->sigma_i[k] : p->sigma;
            r[2] = p->kappa_i ? p->kappa_i[k] : p->kappa;
            r[3] = p->eta_i ? p->eta_i[k] : p->eta;
            r[4] = p->delta_t_i ? p->delta_t_i[k] : p->delta_t;
            const int N = p->N_i ? p->N_i[k] : p->N;
            r[5] = (double)N;
            r[6] = (p->option_type == HADI_PUT) ? p->strike_i[k] : 0.0;
            r[7] = (p->option_type == HADI_PUT) ? 1.0 : 0.0;
            d.Nmax = std::max(d.Nmax, N);
        }
}

// v-grids of all `n` instances rebuilt ON THE DEVICE, each for its own V_0 (v0i: host vector of n values): what every
// team of the reference does in-kernel (rebuild_variance_views, grid_pod.hpp:25-73; call sites use V = 5, d = 5/500,
// jacobian_computation.cpp:253).  Results in c->g_v / c->g_dv; c->v0_i keeps the per-instance V_0 for the price pick.
int rebuild_v_device(Ctx *c, int n, int m2, const std::vector<double> &v0i) {
    int rc;
    if ((rc = ensure(c, c->v0_i, (size_t)n * 8)) || (rc = ensure(c, c->g_v, (size_t)n * (m2 + 1) * 8)) ||
        (rc = ensure(c, c->g_dv, (size_t)n * m2 * 8)))
        return rc;
    if ((rc = stage_to_device(c, c->v0_i.p, v0i.data(), (size_t)n * 8))) return rc;
    hipLaunchKernelGGL(hadi_rebuild_variance_kernel, dim3(n), dim3(256), (size_t)2 * (m2 + 1) * sizeof(double), c->stream, m2, n,
                       ptr<double>(c->v0_i), 5.0, 5.0 / 500, ptr<double>(c->g_v), ptr<double>(c->g_dv));
    HIP_TRY(c, hipGetLastError());
    return HADI_OK;
}

// v-grids built on the host (glibc sinh/asinh, bit-identical to the reference's host-side Grid) for the n_grids values v0[] and
// broadcast to the n instances: instance k takes grid d_sel[k] (device selector; null: all take grid 0).  Results in c->g_v / c->g_dv.
int rebuild_v_host(Ctx *c, int n, int m2, int n_grids, const double *v0, const int *d_sel) {
    std::vector<double> hv((size_t)n_grids * (m2 + 1)), hdv((size_t)n_grids * m2);
    for (int g = 0; g < n_grids; g++) build_v(m2, v0[g], 5.0, 5.0 / 500, hv.data() + (size_t)g * (m2 + 1), hdv.data() + (size_t)g * m2);
    int rc;
    if ((rc = ensure(c, c->src_v, hv.size() * 8)) || (rc = ensure(c, c->src_dv, hdv.size() * 8)) ||
        (rc = ensure(c, c->g_v, (size_t)n * (m2 + 1) * 8)) || (rc = ensure(c, c->g_dv, (size_t)n * m2 * 8)))
        return rc;
    if ((rc = stage_to_device(c, c->src_v.p, hv.data(), hv.size() * 8)) || (rc = stage_to_device(c, c->src_dv.p, hdv.data(), hdv.size() * 8)))
        return rc;
    hipLaunchKernelGGL(hadi_bcast_rows_kernel, dim3(grid1d((size_t)n * (m2 + 1))), dim3(256), 0, c->stream, m2 + 1, n,
                       ptr<double>(c->src_v), d_sel, ptr<double>(c->g_v));
    hipLaunchKernelGGL(hadi_bcast_rows_kernel, dim3(grid1d((size_t)n * m2)), dim3(256), 0, c->stream, m2, n,
                       ptr<double>(c->src_dv), d_sel, ptr<double>(c->g_dv));
    return HADI_OK;
}

// The problem's own arrays to the device (host memory is staged into the library's buffers): the s-grids, the v-grids -- the
// caller's or, with o.rebuild_v, rebuilt for V_0 / V_0_i --, then U and U_0.  *per_inst_v0: the v-grids were rebuilt on the
// device, and c->v0_i holds every instance's V_0 for the price pick.
int stage_problem(Ctx *c, const hadi_problem *p, const CallOut &o, SweepDesc &d, bool *per_inst_v0) {
    const int n = p->n_instances, m1 = p->m1, m2 = p->m2;
    const size_t m = (size_t)(m1 + 1) * (m2 + 1);
    int rc;
    if ((rc = to_device(c, p->memspace, p->vec_s, (size_t)n * (m1 + 1), c->g_s, &d.d_vec_s))) return rc;
    if ((rc = to_device(c, p->memspace, p->delta_s, (size_t)n * m1, c->g_ds, &d.d_delta_s))) return rc;
    *per_inst_v0 = o.rebuild_v && c->t.device_vgrid;
    if (o.rebuild_v && !c->t.device_vgrid && p->V_0_i)
        return fail(c, HADI_ERR_INVALID, "V_0_i needs the device v-grid rebuild (hadi_set_tuning \"device_vgrid\", 1)");
    if (*per_inst_v0) {
        std::vector<double> v0i(n);
        for (int k = 0; k < n; k++) v0i[k] = p->V_0_i ? p->V_0_i[k] : o.V_0;
        rc = rebuild_v_device(c, n, m2, v0i);
    } else if (o.rebuild_v) {
        rc = rebuild_v_host(c, n, m2, 1, &o.V_0, nullptr);
    } else {
        if ((rc = to_device(c, p->memspace, p->vec_v, (size_t)n * (m2 + 1), c->g_v, &d.d_vec_v))) return rc;
        rc = to_device(c, p->memspace, p->delta_v, (size_t)n * m2, c->g_dv, &d.d_delta_v);
    }
    if (rc) return rc;
    if (o.rebuild_v) { d.d_vec_v = ptr<double>(c->g_v); d.d_delta_v = ptr<double>(c->g_dv); }
    if ((rc = to_device(c, p->memspace, p->U, n * m, c->natU, &d.d_natU))) return rc;
    return to_device(c, p->memspace, p->U_0, n * m, c->natU0, &d.d_natU0);
}

// What the status words that a call's last kernels leave on the device mean.
enum StatusKind { STATUS_NONE, STATUS_NODE, STATUS_GREEKS, STATUS_SAMPLES };

// The end of every call: the status words back (c->status, one per instance: hadi_locate_kernel, hadi_pick_kernel and
// hadi_greeks_kernel; sample flags: one per instance and sample), finish_timing -- whose stream synchronisation completes the copy --
// and then the first non-zero word of the leading n_count instances as the call's error (the groups of a Jacobian repeat the
// caller's instances).  pinned: the words come back through the pinned arena, so that the copy does not block the host.
int finish_call(Ctx *c, const SweepDesc &d, const CallOut &o, StatusKind kind, int n_count, bool pinned) {
    const size_t per = kind == STATUS_SAMPLES ? d.n_samp : 1, words = kind == STATUS_NONE ? 0 : d.n * per;
    std::vector<int> pageable;
    int *hs = pinned ? static_cast<int *>(pin_alloc(c, words * sizeof(int))) : nullptr;
    if (!hs) { pageable.resize(words); hs = pageable.data(); }
    if (words)
        HIP_TRY(c, hipMemcpyAsync(hs, kind == STATUS_SAMPLES ? samp_flags(c, d) : ptr<int>(c->status), words * sizeof(int),
                                  hipMemcpyDeviceToHost, c->stream));
    // a cliquet call: the reference nodes' status words as well (pageable: n words, once per call)
    std::vector<int> fixs(d.fix.n_ex > 0 && !d.debug ? (size_t)d.n : 0);
    if (!fixs.empty()) HIP_TRY(c, hipMemcpyAsync(fixs.data(), fix_status(c, d), fixs.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    // a Bates call with a shared matrix: the word of the caller's promise (pageable: one word, once per call)
    int jstat = 0;
    if (d.jmp_shared && !d.debug) HIP_TRY(c, hipMemcpyAsync(&jstat, c->jmp_stat.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipGetLastError());
    const int rc = finish_timing(c, d);
    if (rc) return rc;
    if (jstat) return fail(c, HADI_ERR_INVALID, "shared_grid is set, but not every instance has instance 0's s-grid");
    for (size_t k = 0; k < fixs.size(); k++)
        if (fixs[k]) return fail(c, HADI_ERR_NOT_ON_GRID, "ref_spot = %.17g is not a node of instance %zu's s-grid", d.fix_ref[k % d.n_src], k % d.n_src);
    if (kind == STATUS_NONE) return rc;
    if (kind == STATUS_SAMPLES) return samples_status(c, hs, n_count * per, d.n_samp);
    for (int k = 0; k < n_count; k++) {
        if (hs[k] && (hs[k] == 1 || kind == STATUS_NODE))
            return fail(c, HADI_ERR_NOT_ON_GRID, "S_0 = %.17g is not a node of instance %d's s-grid", o.S_0, k);
        if (hs[k]) return fail(c, HADI_ERR_NOT_ON_GRID, "V_0 = %.17g is not a node of instance %d's v-grid", o.V_0, k);
    }
    return HADI_OK;
}

// Shared driver of hadi_DO_timestepping / hadi_parallel_DO_solve / hadi_compute_base_prices* and the diagnostics
// (x.debug != 0: p->U is input only, the pass's result goes to x.debug_out).
// Ladder (x.ladder; hadi_maturity_ladder, hadi_compute_base_prices_ladder): o.prices is [n][n_snap], the snapshots the sweep
// took on the way ([n][n_snap][n_samp] for a sample call); p->U and p->lambda_bar are not written.
int solve_common(Ctx *c, const hadi_problem *p, const CallExtras &x, const CallOut &o) {
    int rc = check_problem(c, p, true, !o.rebuild_v);
    if (rc || (rc = check_extras(c, p, x, o.prices))) return rc;
    const int debug = x.debug;
    if (debug && !x.debug_out) return fail(c, HADI_ERR_INVALID, "output array missing");
    if (debug && (p->scheme != HADI_SCHEME_DOUGLAS || p->state_precision != HADI_STATE_FP64))
        return fail(c, HADI_ERR_UNSUPPORTED, "diagnostics cover fp64 Douglas steps");
    if (debug == 2 && p->variant != HADI_EU && p->variant != HADI_DIV)
        return fail(c, HADI_ERR_UNSUPPORTED, "hadi_debug_col_solve is the plain A2 solve (no projection): European variants only");
    DeviceGuard guard(c->device);
    pin_rewind(c);
    const int n = p->n_instances, m1 = p->m1, m2 = p->m2;
    const size_t m = (size_t)(m1 + 1) * (m2 + 1);
    SweepDesc d;
    fill_desc(p, d, 1);
    if (debug == 1 && (x.debug_step < 1 || x.debug_step > d.Nmax))
        return fail(c, HADI_ERR_INVALID, "step %d outside 1..%d", x.debug_step, d.Nmax);
    bool per_inst_v0;
    if ((rc = stage_problem(c, p, o, d, &per_inst_v0))) return rc;
    // the buffers the outputs pass through, grown before the sweep: growing one after it would drop the loop it just captured
    if (p->memspace != HADI_MEM_DEVICE && (rc = ensure(c, c->natOut, n * m * 8))) return rc;
    if (o.pick && ((rc = ensure(c, c->prices, n * 8)) || (rc = ensure(c, c->status, n * sizeof(int))))) return rc;
    const double *const d_v0_i = per_inst_v0 ? ptr<double>(c->v0_i) : nullptr;
    apply_extras(d, x, o, d_v0_i);
    HadiPlan pl;
    if ((rc = run_sweep(c, d, pl))) return rc;

    if (x.ladder) {  // the snapshots and the locate step's status words (or the samples and their flag words) are all that leaves
        const DevBuf &src = d.n_samp > 0 ? c->samp_out : c->snap_out;
        if ((rc = from_device(c, p->memspace, o.prices, static_cast<const double *>(src.p), (size_t)n * d.n_snap * std::max(d.n_samp, 1))))
            return rc;
        return finish_call(c, d, o, d.n_samp > 0 ? STATUS_SAMPLES : STATUS_NODE, n, false);
    }

    // solution back to the caller's U (natural layout); diagnostics: the pass's result to debug_out, U untouched
    double *const host_dst = debug ? x.debug_out : p->U;
    double *const d_out = p->memspace == HADI_MEM_DEVICE ? host_dst : ptr<double>(c->natOut);
    hipLaunchKernelGGL(hadi_unpack_kernel, dim3(grid1d(n * m)), dim3(256), 0, c->stream, pl.L, n,
                       debug == 1 ? ptr<double>(c->Y) : ptr<double>(c->U), d_out);
    if (p->memspace == HADI_MEM_HOST && (rc = from_device(c, p->memspace, host_dst, d_out, n * m))) return rc;
    const bool american = (p->variant == HADI_AM || p->variant == HADI_AM_DIV) && !debug;
    if (american && p->lambda_bar) {
        double *d_l;
        if (p->memspace == HADI_MEM_DEVICE) d_l = p->lambda_bar;
        else {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            d_l = ptr<double>(c->natOut);
        }
        hipLaunchKernelGGL(hadi_unpack_kernel, dim3(grid1d(n * m)), dim3(256), 0, c->stream, pl.L, n, ptr<double>(c->LAM), d_l);
        if (p->memspace == HADI_MEM_HOST && (rc = from_device(c, p->memspace, p->lambda_bar, d_l, n * m))) return rc;
    }
    if (o.pick) {
        hipLaunchKernelGGL(hadi_pick_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, pl.L, n, d.d_vec_s, d.d_vec_v,
                           ptr<double>(c->U), o.S_0, d_v0_i, o.V_0, ptr<double>(c->prices), 1, ptr<int>(c->status));
        if ((rc = from_device(c, p->memspace, o.prices, ptr<double>(c->prices), n))) return rc;
    }
    return finish_call(c, d, o, o.pick ? STATUS_NODE : STATUS_NONE, n, false);
}

// hadi_compute_greeks: the sweep of hadi_DO_timestepping on the caller's grids, then hadi_greeks_kernel on the packed state the
// sweep left in the handle (every execution path of run_sweep ends with an explicit U, American sweeps with an explicit
// lambda_bar as well) and on its operator tables.  No field is unpacked or copied; p->U and p->lambda_bar are not written.
static_assert(HADI_GK_N == HADI_N_GREEKS && HADI_GK_LAMBDA == HADI_GREEK_LAMBDA && HADI_GK_THETA == HADI_GREEK_THETA, "hadi.h / hadi_k_greeks.h columns");
int greeks_common(Ctx *c, const hadi_problem *p, const CallOut &o) {
    int rc = check_problem(c, p, true, true);
    if (rc) return rc;
    if (!o.greeks) return fail(c, HADI_ERR_INVALID, "greeks missing");
    if (p->state_precision == HADI_STATE_FP32)
        return fail(c, HADI_ERR_UNSUPPORTED, "Greeks need the fp64 state: second-derivative stencils have weight sums near 1e2 on 512x256, "
                                             "which turn a state rounded to 24 bits into noise");
    DeviceGuard guard(c->device);
    pin_rewind(c);
    const int n = p->n_instances, m1 = p->m1;
    SweepDesc d;
    fill_desc(p, d, 1);
    bool per_inst_v0;
    if ((rc = stage_problem(c, p, o, d, &per_inst_v0))) return rc;
    // the buffers the outputs pass through, grown before the sweep: growing one after it would drop the loop it just captured
    const size_t nlad = (size_t)n * (m1 + 1) * HADI_GK_N;
    if ((rc = ensure(c, c->prices, (size_t)n * HADI_GK_N * 8)) || (rc = ensure(c, c->status, n * sizeof(int)))) return rc;
    if (o.ladder && (rc = ensure(c, c->natOut, nlad * 8))) return rc;

    HadiPlan pl;
    if ((rc = run_sweep(c, d, pl))) return rc;

    const HadiLayout &L = pl.L;
    const bool american = p->variant == HADI_AM || p->variant == HADI_AM_DIV;
    HadiGreeksArgs g;
    g.L = L; g.n_inst = n; g.american = american ? 1 : 0;
    g.ntiles = L.B == 1 ? (m1 + HADI_GK_TILE) / HADI_GK_TILE : 1;
    g.span = L.B == 1 ? HADI_GK_TILE + 2 * HADI_GK_HALO : L.rowp;
    g.U = ptr<double>(c->U); g.LAM = american ? ptr<double>(c->LAM) : nullptr;
    g.scoef = ptr<double>(c->scoef); g.b2row = ptr<double>(c->b2row); g.rowc = ptr<double>(c->rowc);
    g.ipar = ptr<HadiInstPar>(c->ipar);
    g.vec_s = d.d_vec_s; g.vec_v = d.d_vec_v; g.delta_s = d.d_delta_s; g.delta_v = d.d_delta_v;
    g.S_0 = o.S_0; g.V_0 = o.V_0;
    g.greeks = ptr<double>(c->prices); g.ladder = o.ladder ? ptr<double>(c->natOut) : nullptr; g.status = ptr<int>(c->status);
    hipLaunchKernelGGL(hadi_greeks_kernel, dim3((unsigned)(n * g.ntiles)), dim3(HADI_GK_THREADS), hadi_greeks_smem(g.span), c->stream, g);
    HIP_TRY(c, hipGetLastError());
    if ((rc = from_device(c, p->memspace, o.greeks, ptr<double>(c->prices), (size_t)n * HADI_GK_N))) return rc;
    if (o.ladder && (rc = from_device(c, p->memspace, o.ladder, ptr<double>(c->natOut), nlad))) return rc;
    return finish_call(c, d, o, STATUS_GREEKS, n, false);
}

// The grids of the G groups of a Jacobian's batch (6, or 9 with the jump columns): the caller's s-rows replicated, the v-grids
// rebuilt for V_0 + eps (group 5) and V_0 (every other group); c->v0_i keeps the per-instance V_0 for the price pick.  n_col: the
// output columns per instance.
int jacobian_grids(Ctx *c, const hadi_problem *p, int G, const CallOut &o, int n_col, SweepDesc &d) {
    const int n0 = p->n_instances, m1 = p->m1, m2 = p->m2, n = n0 * G;
    int rc;
    const double *src_s, *src_ds;
    // (natOut stages delta_s here and takes J and the base prices after the sweep; prices / status: the pick.  All grown before
    // the sweep: growing one after it would drop the loop it just captured)
    if ((rc = ensure(c, c->natOut, (size_t)n0 * std::max(m1, G * std::max(n_col, 1)) * 8)) || (rc = ensure(c, c->prices, n * 8)) ||
        (rc = ensure(c, c->status, n * sizeof(int))))
        return rc;
    if ((rc = to_device(c, p->memspace, p->vec_s, (size_t)n0 * (m1 + 1), c->natU, &src_s))) return rc;
    if ((rc = to_device(c, p->memspace, p->delta_s, (size_t)n0 * m1, c->natOut, &src_ds))) return rc;
    std::vector<int> sel_a(n), sel_b(n);
    std::vector<double> v0i(n);
    for (int g = 0; g < G; g++)
        for (int k = 0; k < n0; k++) {
            sel_a[g * n0 + k] = k;
            sel_b[g * n0 + k] = (g == 5) ? 1 : 0;
            const double v0k = p->V_0_i ? p->V_0_i[k] : o.V_0;
            v0i[g * n0 + k] = (g == 5) ? v0k + o.eps : v0k;
        }
    if ((rc = ensure(c, c->sel_a, n * sizeof(int))) || (rc = ensure(c, c->sel_b, n * sizeof(int))) ||
        (rc = ensure(c, c->v0_i, n * 8)) || (rc = ensure(c, c->src_v, 2 * (m2 + 1) * 8)) ||
        (rc = ensure(c, c->src_dv, 2 * m2 * 8)) || (rc = ensure(c, c->g_s, (size_t)n * (m1 + 1) * 8)) ||
        (rc = ensure(c, c->g_ds, (size_t)n * m1 * 8)) || (rc = ensure(c, c->g_v, (size_t)n * (m2 + 1) * 8)) ||
        (rc = ensure(c, c->g_dv, (size_t)n * m2 * 8)))
        return rc;  // (all grown here, ahead of the first launch, in one order whichever way the v-grids are rebuilt)
    hipStream_t s = c->stream;
    if ((rc = stage_to_device(c, c->sel_a.p, sel_a.data(), n * sizeof(int)))) return rc;
    hipLaunchKernelGGL(hadi_bcast_rows_kernel, dim3(grid1d((size_t)n * (m1 + 1))), dim3(256), 0, s, m1 + 1, n, src_s,
                       ptr<int>(c->sel_a), ptr<double>(c->g_s));
    hipLaunchKernelGGL(hadi_bcast_rows_kernel, dim3(grid1d((size_t)n * m1)), dim3(256), 0, s, m1, n, src_ds,
                       ptr<int>(c->sel_a), ptr<double>(c->g_ds));
    if (c->t.device_vgrid) {
        // every instance rebuilds its own v-grid on the device: V_0 + eps for group 5, V_0 for the others
        // (jacobian_computation.cpp:253,339-341)
        if ((rc = rebuild_v_device(c, n, m2, v0i))) return rc;
    } else {
        const double v0[2] = {o.V_0, o.V_0 + o.eps};
        if ((rc = stage_to_device(c, c->sel_b.p, sel_b.data(), n * sizeof(int))) || (rc = stage_to_device(c, c->v0_i.p, v0i.data(), (size_t)n * 8)) ||
            (rc = rebuild_v_host(c, n, m2, 2, v0, ptr<int>(c->sel_b))))
            return rc;
    }
    // (no synchronisation here: the host vectors above went through the pinned arena, and the device-side staging buffers natU /
    // natOut are only reused by later operations of the same stream)
    d.d_vec_s = ptr<double>(c->g_s); d.d_delta_s = ptr<double>(c->g_ds);
    d.d_vec_v = ptr<double>(c->g_v); d.d_delta_v = ptr<double>(c->g_dv);
    return HADI_OK;
}

// compute_jacobian*: the reference runs 6 solves one after the other inside each team
// (jacobian_computation.cpp:232-363); here they are 6n independent instances of ONE batched sweep:
// group 0 = base, 1..4 = kappa, eta, sigma, rho + eps, 5 = v-grid rebuilt for V_0 + eps.
// Ladder (x.ladder; hadi_compute_jacobian_ladder): J [n][n_snap][5] and base_prices [n][n_snap] from the snapshots of the 6n solves.
int jacobian_common(Ctx *c, const hadi_problem *p, const CallExtras &x, const CallOut &o) {
    int rc = check_problem(c, p, false, false);
    if (rc || (rc = check_extras(c, p, x, (o.J && o.base_prices) ? o.J : nullptr))) return rc;
    const int n_samp = x.sampled ? x.samples->n_samp : 0;
    const int n_col = x.n_snap * std::max(n_samp, 1);  // columns per instance: a sample call's [n_snap][n_samp] is the ladder's [n_snap]
    DeviceGuard guard(c->device);
    pin_rewind(c);
    if (!p->U_0) return fail(c, HADI_ERR_INVALID, "U_0 (initial condition) is required for the Jacobian");
    if (!o.J || !o.base_prices) return fail(c, HADI_ERR_INVALID, "J / base_prices missing");
    // G groups, NC = G - 1 columns: the five Heston parameters, and with x.jump_cols lambda (6), mu_J (7), sigma_J (8)
    const int n0 = p->n_instances, m1 = p->m1, m2 = p->m2, G = x.jump_cols ? HADI_JUMP_GROUPS : 6, NC = G - 1;
    if (!c->t.device_vgrid && p->V_0_i)
        return fail(c, HADI_ERR_INVALID, "V_0_i needs the device v-grid rebuild (hadi_set_tuning \"device_vgrid\", 1)");
    const int n = n0 * G;
    const size_t m = (size_t)(m1 + 1) * (m2 + 1);
    const double eps = o.eps;
    SweepDesc d;
    fill_desc(p, d, G);
    for (int k = 0; k < n0; k++) {
        d.par8[((size_t)1 * n0 + k) * 8 + 2] += eps;  // kappa
        d.par8[((size_t)2 * n0 + k) * 8 + 3] += eps;  // eta
        d.par8[((size_t)3 * n0 + k) * 8 + 1] += eps;  // sigma
        d.par8[((size_t)4 * n0 + k) * 8 + 0] += eps;  // rho
    }
    if ((rc = jacobian_grids(c, p, G, o, n_col, d))) return rc;
    hipStream_t s = c->stream;
    // every solve starts from U_0 (jacobian_computation.cpp:307-309); payoff for American = U_0 too
    if ((rc = to_device(c, p->memspace, p->U_0, n0 * m, c->natU0, &d.d_natU))) return rc;
    d.d_natU0 = d.d_natU;
    apply_extras(d, x, o, ptr<double>(c->v0_i));

    HadiPlan pl;
    if ((rc = run_sweep(c, d, pl))) return rc;
    if (!x.ladder)
        hipLaunchKernelGGL(hadi_pick_kernel, dim3((n + 63) / 64), dim3(64), 0, s, pl.L, n, d.d_vec_s, d.d_vec_v,
                           ptr<double>(c->U), o.S_0, ptr<double>(c->v0_i), o.V_0, ptr<double>(c->prices), 1, ptr<int>(c->status));
    // J(k, param) = (pert - base) / eps on the device (jacobian_computation.cpp:329,360): with HADI_MEM_DEVICE the rows
    // never leave HBM (hadi_lm_partials_device reduces them there); only the n status words come back
    double *dJ = o.J, *db = o.base_prices;
    if (p->memspace == HADI_MEM_HOST) {
        dJ = ptr<double>(c->natOut);
        db = dJ + (size_t)n0 * NC * std::max(n_col, 1);
    }
    const size_t nrow = (size_t)n0 * std::max(n_col, 1);  // rows of J
    if (x.ladder)  // (a sample call: the same kernel with n_snap * n_samp columns)
        hipLaunchKernelGGL(hadi_jacobian_ladder_rows_kernel, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, s, n0, n_col, NC,
                           n_samp > 0 ? ptr<double>(c->samp_out) : ptr<double>(c->snap_out), eps, dJ, db);
    else if (x.jump_cols)
        hipLaunchKernelGGL(hadi_jacobian_rows8_kernel, dim3((n0 + 255) / 256), dim3(256), 0, s, n0, ptr<double>(c->prices), eps, dJ, db);
    else
        hipLaunchKernelGGL(hadi_jacobian_rows_kernel, dim3((n0 + 255) / 256), dim3(256), 0, s, n0, ptr<double>(c->prices), eps, dJ, db);
    if (p->memspace == HADI_MEM_HOST) {
        HIP_TRY(c, hipMemcpyAsync(o.J, dJ, nrow * NC * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(o.base_prices, db, nrow * 8, hipMemcpyDeviceToHost, s));
    }
    // (a sample call: the v0 group located its own row and the s-grids are the same, so the caller's n0 instances decide as well)
    return finish_call(c, d, o, n_samp > 0 ? STATUS_SAMPLES : STATUS_NODE, n0, n_samp == 0);
}

int with_variant(hadi_ctx *ctx, const hadi_problem *p, int variant, hadi_problem *tmp) {
    if (!ctx) return HADI_ERR_INVALID;
    if (!p) return fail(reinterpret_cast<Ctx *>(ctx), HADI_ERR_INVALID, "problem is NULL");
    *tmp = *p;
    tmp->variant = variant;
    return HADI_OK;
}

// Frees everything a (possibly half-built) handle owns.  The caller has made the handle's device current.
void release_handle(Ctx *c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf *bufs[] = {&c->U, &c->Y, &c->LAM, &c->U0, &c->UT, &c->scoef, &c->b2row, &c->rowc, &c->a2i, &c->pb,
                      &c->rinv, &c->rwork, &c->ipar, &c->par8, &c->g_s, &c->g_v, &c->g_ds, &c->g_dv, &c->src_v,
                      &c->src_dv, &c->sel_a, &c->sel_b, &c->v0_i, &c->natU, &c->natU0, &c->natOut, &c->prices,
                      &c->status, &c->div_flag, &c->div_amt, &c->div_pct, &c->V, &c->R1, &c->C2, &c->pay_mis, &c->Uf, &c->Yf,
                      &c->order, &c->lm31, &c->team, &c->rs_tab, &c->snap_steps, &c->snap_node, &c->snap_out, &c->samp_in, &c->samp_tap, &c->samp_out, &c->ex_flag,
                      &c->ko_flag, &c->ko_bounds, &c->ko_iab, &c->ko_rebate, &c->jmp_G, &c->jmp_a, &c->jmp_par, &c->jmp_stat, &c->jmp_mat,
                      &c->fix_flag, &c->fix_w, &c->fix_ref, &c->fix_iref, &c->fix_mode, &c->fix_c};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (auto &g : c->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    for (auto e : c->kev) (void)hipEventDestroy(e);
    for (auto e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->wait_ev) (void)hipEventDestroy(c->wait_ev);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->err_host) (void)hipHostFree(c->err_host);
    if (c->pin) (void)hipHostFree(c->pin);
    delete c;
}

}  // namespace

// =====================================================================================================
extern "C" {

int hadi_version(void) { return HADI_VERSION_MAJOR * 100 + HADI_VERSION_MINOR; }

#if defined(HADI_TEAM_STAMPS)
// diagnostic build only (tools/team_stamps.py): the 16 phase stamps of the last instance-resident launch
int hadi_debug_team_stamps(hadi_ctx *ctx, unsigned long long *out16) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c || !c->team.p) return 1;
    return hipMemcpy(out16, ptr<int>(c->team) + 384, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess;
}
#endif

#if defined(HADI_STAMPS)
// diagnostic build only (tools/stamps.py)
int hadi_debug_stamps(unsigned long long *out32, int reset) {
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_hadi_stamps), 32 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_hadi_stamps), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

const char *hadi_status_string(int s) {
    switch (s) {
        case HADI_OK: return "ok";
        case HADI_ERR_INVALID: return "invalid argument";
        case HADI_ERR_UNSUPPORTED: return "unsupported grid shape";
        case HADI_ERR_HIP: return "HIP runtime error";
        case HADI_ERR_NOT_ON_GRID: return "S_0 is not a grid node";
        case HADI_ERR_NO_DEVICE: return "no usable gfx950 GPU (libhadi has no CPU path)";
        case HADI_ERR_ALLOC: return "device allocation failed";
        case HADI_ERR_INTERNAL: return "device-side failure reported by a kernel (results invalid)";
        default: return "unknown";
    }
}

int hadi_create(hadi_ctx **out, int device_id) {
    if (!out) return HADI_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return HADI_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return HADI_ERR_INVALID;
    DeviceGuard guard(device_id);  // the caller's current device is left as it was found
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return HADI_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HADI_ERR_NO_DEVICE;  // code object is gfx950-only
    Ctx *c = new Ctx;
    c->device = device_id;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->name = prop.name;
    c->arch = prop.gcnArchName;
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming) == hipSuccess;
    hadi_for_each_kernel([&](auto kernel) { ok = ok && raise_lds_limit(kernel) == hipSuccess; });
    ok = ok && raise_lds_limit(hadi_jump_kernel) == hipSuccess;  // (its strip of G: 66 KiB at m1 = 512, 132 KiB at m1 = 1024)
    ok = ok && raise_lds_limit(hadi_jump_sel_kernel) == hipSuccess;       // (the same strip)
    ok = ok && raise_lds_limit(hadi_lm_partials_n_kernel) == hipSuccess;  // (45 rows of 256 doubles at n_par = 8: 90 KiB)
    for (auto &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->wait_ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&c->err_host), 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (ok) {
        c->pin_want = (size_t)1 << 20;  // 1 MB to start with (3000 instances' parameter rows are 192 KB)
        pin_rewind(c);
        *c->err_host = 0;
        ok = hipHostGetDevicePointer(reinterpret_cast<void **>(&c->err_dev), c->err_host, 0) == hipSuccess;
    }
    if (!ok) {  // one way out: whatever was created is released
        release_handle(c);
        return HADI_ERR_HIP;
    }
    *out = reinterpret_cast<hadi_ctx *>(c);
    return HADI_OK;
}

int hadi_destroy(hadi_ctx *ctx) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_OK;
    DeviceGuard guard(c->device);
    release_handle(c);
    return HADI_OK;
}

const char *hadi_last_error(const hadi_ctx *ctx) {
    const Ctx *c = reinterpret_cast<const Ctx *>(ctx);
    return c ? c->err.c_str() : "null handle";
}

int hadi_set_profiling(hadi_ctx *ctx, int enabled) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    c->profiling = enabled ? 1 : 0;
    return HADI_OK;
}

// The keys, their fields and normalisations: hadi_tuning_key (csrc/hadi_route.h).  Here: the four read-only counters, and
// "team_launch", which clears team_failed when set and reads back as -2 once a team has failed.
static const unsigned long long *graph_counter(const Ctx *c, const char *key) {
    return !std::strcmp(key, "graph_captures") ? &c->graph_captures : !std::strcmp(key, "graph_replays") ? &c->graph_replays :
           !std::strcmp(key, "graph_drops") ? &c->graph_drops : !std::strcmp(key, "graph_evictions") ? &c->graph_evictions : nullptr;
}

int hadi_set_tuning(hadi_ctx *ctx, const char *key, int value) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c || !key) return HADI_ERR_INVALID;
    if (graph_counter(c, key)) return fail(c, HADI_ERR_INVALID, "'%s' is a read-only counter", key);
    const HadiTuneKey *e = hadi_tuning_key(key);
    if (!e) return fail(c, HADI_ERR_INVALID, "unknown tuning key '%s'", key);
    const char *refused = hadi_tuning_set(c->t, *e, value);
    if (refused) return fail(c, HADI_ERR_INVALID, refused, key);
    if (e->f == &HadiHandleTuning::team_launch) c->team_failed = 0;
    return HADI_OK;
}

int hadi_get_tuning(const hadi_ctx *ctx, const char *key, int *value) {
    const Ctx *c = reinterpret_cast<const Ctx *>(ctx);
    if (!c || !key || !value) return HADI_ERR_INVALID;
    const HadiTuneKey *e = hadi_tuning_key(key);
    if (const unsigned long long *n = graph_counter(c, key)) *value = (int)std::min<unsigned long long>(*n, INT_MAX);
    else if (!e) return HADI_ERR_INVALID;
    else if (e->f == &HadiHandleTuning::team_launch && c->team_failed) *value = -2;
    else *value = hadi_tuning_word(c->t, *e);
    return HADI_OK;
}

int hadi_wait_stream(hadi_ctx *ctx, void *producer_stream) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    DeviceGuard guard(c->device);
    HIP_TRY(c, hipEventRecord(c->wait_ev, static_cast<hipStream_t>(producer_stream)));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->wait_ev, 0));
    return HADI_OK;
}

int hadi_get_timing(const hadi_ctx *ctx, hadi_timing *out) {
    const Ctx *c = reinterpret_cast<const Ctx *>(ctx);
    if (!c || !out) return HADI_ERR_INVALID;
    *out = c->timing;
    return HADI_OK;
}

int hadi_device_info(const hadi_ctx *ctx, char *name, int name_len, int *compute_units, char *arch, int arch_len) {
    const Ctx *c = reinterpret_cast<const Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    if (name && name_len > 0) std::snprintf(name, name_len, "%s", c->name.c_str());
    if (arch && arch_len > 0) std::snprintf(arch, arch_len, "%s", c->arch.c_str());
    if (compute_units) *compute_units = c->cu_count;
    return HADI_OK;
}

int hadi_describe_last_sweep(const hadi_ctx *ctx, char *buf, int len) {
    const Ctx *c = reinterpret_cast<const Ctx *>(ctx);
    if (!c || !buf || len <= 0) return HADI_ERR_INVALID;
    std::snprintf(buf, len, "%s", c->last_path.c_str());
    return HADI_OK;
}

void *hadi_stream(hadi_ctx *ctx) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    return c ? (void *)c->stream : nullptr;
}

// ---- grids ------------------------------------------------------------------------------------------
int hadi_make_grid(int m1, double S, double S_0, double K, double cc, int m2, double V, double V_0, double d,
                   double *vec_s, double *vec_v, double *delta_s, double *delta_v) {
    if (m1 < 1 || m2 < 1 || !vec_s || !vec_v || !delta_s || !delta_v) return HADI_ERR_INVALID;
    const double lo = std::asinh(-K / cc);
    const double Delta_xi = (1.0 / m1) * (std::asinh((S - K) / cc) - lo);
    for (int i = 0; i <= m1; i++) vec_s[i] = K + cc * std::sinh(lo + i * Delta_xi);
    sorted_insert_drop_largest(vec_s, m1 + 1, S_0);
    for (int i = 0; i < m1; i++) delta_s[i] = vec_s[i + 1] - vec_s[i];
    build_v(m2, V_0, V, d, vec_v, delta_v);
    return HADI_OK;
}

int hadi_rebuild_variance(int m2, double V_0_new, double V, double d, double *vec_v, double *delta_v) {
    if (m2 < 1 || !vec_v || !delta_v) return HADI_ERR_INVALID;
    build_v(m2, V_0_new, V, d, vec_v, delta_v);
    return HADI_OK;
}

int hadi_find_s_index(int m1, const double *vec_s, double S_0) {
    for (int i = 0; i <= m1; i++)
        if (std::fabs(vec_s[i] - S_0) < 1e-10) return i;
    return -1;
}

int hadi_find_v_index(int m2, const double *vec_v, double V_0) {
    for (int i = 0; i <= m2; i++)
        if (std::fabs(vec_v[i] - V_0) < 1e-10) return i;
    return 0;
}

// ---- hot path ------------------------------------------------------------------------------------------
int hadi_DO_timestepping(hadi_ctx *ctx, const hadi_problem *p) {
    return solve_common(reinterpret_cast<Ctx *>(ctx), p, CallExtras{}, CallOut{});
}

int hadi_parallel_DO_solve(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !base_prices) return fail(c, HADI_ERR_INVALID, "base_prices missing");
    CallOut o; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = base_prices;
    return solve_common(c, p, CallExtras{}, o);
}

int hadi_compute_greeks(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double *greeks, double *ladder) {
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.greeks = greeks; o.ladder = ladder;
    return greeks_common(reinterpret_cast<Ctx *>(ctx), p, o);
}

int hadi_compute_base_prices(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !base_prices) return fail(c, HADI_ERR_INVALID, "base_prices missing");
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = base_prices;
    return solve_common(c, p, CallExtras{}, o);
}

int hadi_debug_row_pass(hadi_ctx *ctx, const hadi_problem *p, int step, double *Y1rhs) {
    CallExtras x; x.debug = 1; x.debug_step = step; x.debug_out = Y1rhs;
    return solve_common(reinterpret_cast<Ctx *>(ctx), p, x, CallOut{});
}

int hadi_debug_col_solve(hadi_ctx *ctx, const hadi_problem *p, double *X) {
    CallExtras x; x.debug = 2; x.debug_out = X;
    return solve_common(reinterpret_cast<Ctx *>(ctx), p, x, CallOut{});
}

int hadi_debug_rcp(hadi_ctx *ctx, int n, const double *x, double *out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    if (n < 1 || !x || !out) return fail(c, HADI_ERR_INVALID, "bad arguments");
    DeviceGuard guard(c->device);
    int rc;
    if ((rc = ensure(c, c->natU, (size_t)n * 8)) || (rc = ensure(c, c->natOut, (size_t)n * 8))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->natU.p, x, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hadi_rcp_kernel, dim3(grid1d((size_t)n)), dim3(256), 0, c->stream, n, ptr<double>(c->natU), ptr<double>(c->natOut));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, c->natOut.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HADI_OK;
}

#define HADI_VARIANT_WRAPPERS(suffix, variant)                                                                   \
    int hadi_compute_base_prices_##suffix(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,          \
                                          double *base_prices) {                                                 \
        hadi_problem t;                                                                                          \
        int rc = with_variant(ctx, p, variant, &t);                                                              \
        return rc ? rc : hadi_compute_base_prices(ctx, &t, S_0, V_0, base_prices);                               \
    }                                                                                                            \
    int hadi_compute_jacobian_##suffix(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, \
                                       double *J, double *base_prices) {                                         \
        hadi_problem t;                                                                                          \
        int rc = with_variant(ctx, p, variant, &t);                                                              \
        return rc ? rc : hadi_compute_jacobian(ctx, &t, S_0, V_0, eps, J, base_prices);                          \
    }

int hadi_compute_jacobian(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, double *J,
                          double *base_prices) {
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(reinterpret_cast<Ctx *>(ctx), p, CallExtras{}, o);
}

// ---- maturity ladder: the sweep's intermediate states at the price node --------------------------------
int hadi_maturity_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_snap, const int *snap_steps, double *prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps;
    CallOut o; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_base_prices_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_snap, const int *snap_steps,
                                    double *prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps;
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, int n_snap,
                                 const int *snap_steps, double *J, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(c, p, x, o);
}

// ---- Bermudan: the European sweep with U <- max(U, payoff) at the end of the listed steps --------------------
int hadi_bermudan_timestepping(hadi_ctx *ctx, const hadi_problem *p, int n_ex, const int *ex_steps, int ex_rows) {
    CallExtras x; x.bermudan = true; x.ex.n_ex = n_ex; x.ex.rows = ex_rows; x.ex.steps = ex_steps;
    return solve_common(reinterpret_cast<Ctx *>(ctx), p, x, CallOut{});
}

int hadi_compute_base_prices_bermudan(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_ex, const int *ex_steps,
                                      int ex_rows, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !base_prices) return fail(c, HADI_ERR_INVALID, "base_prices missing");
    CallExtras x; x.bermudan = true; x.ex.n_ex = n_ex; x.ex.rows = ex_rows; x.ex.steps = ex_steps;
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = base_prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_bermudan(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, int n_ex,
                                   const int *ex_steps, int ex_rows, double *J, double *base_prices) {
    CallExtras x; x.bermudan = true; x.ex.n_ex = n_ex; x.ex.rows = ex_rows; x.ex.steps = ex_steps;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(reinterpret_cast<Ctx *>(ctx), p, x, o);
}

// ---- Bates: the European sweep with the jump sub-step U <- U + lambda dt G U at the end of every step ------------------------
int hadi_bates_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_jumps *jumps) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    CallExtras x; x.jumps = jumps;
    return solve_common(c, p, x, CallOut{});
}

int hadi_compute_base_prices_bates(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_jumps *jumps, double *prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (!jumps || !prices)) return fail(c, HADI_ERR_INVALID, "%s missing", jumps ? "prices" : "jump description");
    CallExtras x; x.jumps = jumps;
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_bates(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_jumps *jumps,
                                double *J, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    CallExtras x; x.jumps = jumps;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(c, p, x, o);
}

// The eight-column Jacobian: kappa, eta, sigma, rho, V_0, lambda, mu_J, sigma_J -- nine groups of one batched sweep.
int hadi_compute_jacobian_bates_jumps(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_jumps *jumps,
                                      double *J, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    CallExtras x; x.jumps = jumps; x.jump_cols = true; x.jump_eps = eps;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(c, p, x, o);
}

// The generator of one grid in natural order, through the kernels the sweep uses (host arrays in and out).
int hadi_debug_jump_matrix(hadi_ctx *ctx, int m1, const double *vec_s, double mu, double sigma, double *G_out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    if (!vec_s || !G_out) return fail(c, HADI_ERR_INVALID, "%s missing", vec_s ? "G_out" : "vec_s");
    if (!std::isfinite(mu) || !std::isfinite(sigma) || !(sigma > 0.0)) return fail(c, HADI_ERR_INVALID, "jump law (%g, %g) is not admissible", mu, sigma);
    HadiPlan pl;
    if (hadi_make_plan(m1, 8, 1, 8 * c->cu_count, &pl, c->t.tune, 8) || pl.row_seq)
        return fail(c, HADI_ERR_UNSUPPORTED, "no streaming layout for m1 = %d", m1);
    DeviceGuard guard(c->device);
    pin_rewind(c);
    const HadiLayout &L = pl.L;
    const size_t m1p = (size_t)m1 + 1, gd = hadi_jump_matrix_doubles(L);
    const double ms[2] = {mu, sigma};
    int rc;
    if ((rc = ensure(c, c->g_s, m1p * 8)) || (rc = ensure(c, c->jmp_G, gd * 8)) || (rc = ensure(c, c->jmp_par, 16)) ||
        (rc = ensure(c, c->natOut, m1p * m1p * 8)))
        return rc;
    if ((rc = stage_to_device(c, c->g_s.p, vec_s, m1p * 8)) || (rc = stage_to_device(c, c->jmp_par.p, ms, 16))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->jmp_G.p, 0, gd * 8, s));
    hipLaunchKernelGGL(hadi_jump_matrix_kernel, dim3((unsigned)((m1p * m1p + 255) / 256)), dim3(256), 0, s, L, 1, ptr<double>(c->g_s),
                       ptr<double>(c->jmp_par), ptr<double>(c->jmp_G));
    hipLaunchKernelGGL(hadi_jump_matrix_unpack_kernel, dim3((unsigned)((m1p * m1p + 255) / 256)), dim3(256), 0, s, L, ptr<double>(c->jmp_G),
                       ptr<double>(c->natOut));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(G_out, c->natOut.p, m1p * m1p * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->pin_dirty = 0;
    return HADI_OK;
}

// ---- knock-out barrier: the European sweep with U <- rebate beyond the barriers at the end of the monitoring steps ----------
int hadi_barrier_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_barrier *barrier) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !barrier) return fail(c, HADI_ERR_INVALID, "barrier description missing");
    CallExtras x; x.barrier = barrier;
    return solve_common(c, p, x, CallOut{});
}

int hadi_compute_base_prices_barrier(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_barrier *barrier,
                                     double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (!barrier || !base_prices)) return fail(c, HADI_ERR_INVALID, "%s missing", barrier ? "base_prices" : "barrier description");
    CallExtras x; x.barrier = barrier;
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = base_prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_barrier(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_barrier *barrier,
                                  double *J, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !barrier) return fail(c, HADI_ERR_INVALID, "barrier description missing");
    CallExtras x; x.barrier = barrier;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(c, p, x, o);
}

// ---- forward-start options and cliquets: the European sweep with strike fixings at the end of the fixing steps ----------------
int hadi_cliquet_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_cliquet *cliquet) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !cliquet) return fail(c, HADI_ERR_INVALID, "cliquet description missing");
    CallExtras x; x.cliquet = cliquet;
    return solve_common(c, p, x, CallOut{});
}

int hadi_compute_base_prices_cliquet(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_cliquet *cliquet,
                                     double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (!cliquet || !base_prices)) return fail(c, HADI_ERR_INVALID, "%s missing", cliquet ? "base_prices" : "cliquet description");
    CallExtras x; x.cliquet = cliquet;
    CallOut o; o.rebuild_v = true; o.pick = true; o.S_0 = S_0; o.V_0 = V_0; o.prices = base_prices;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_cliquet(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_cliquet *cliquet,
                                  double *J, double *base_prices) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !cliquet) return fail(c, HADI_ERR_INVALID, "cliquet description missing");
    CallExtras x; x.cliquet = cliquet;
    CallOut o; o.S_0 = S_0; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base_prices;
    return jacobian_common(c, p, x, o);
}

// ---- sampled ladder: the ladder's calls with n_samp interpolants of the row of V_0 in the single node's place --------------
int hadi_sample_ladder(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap, const int *snap_steps,
                       double *out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples;
    CallOut o; o.pick = true; o.V_0 = V_0; o.prices = out;
    return solve_common(c, p, x, o);
}

int hadi_compute_base_prices_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                                     const int *snap_steps, double *out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples;
    CallOut o; o.rebuild_v = true; o.pick = true; o.V_0 = V_0; o.prices = out;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, double eps, const hadi_samples *samples, int n_snap,
                                  const int *snap_steps, double *J, double *base) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples;
    CallOut o; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base;
    return jacobian_common(c, p, x, o);
}

// ---- Bates surface: the sample calls with the jump sub-step at the end of every step, behind the step's last column pass and in
// front of the snapshot.  Both features' fields of CallExtras are filled; nothing else is new.
int hadi_bates_sample_ladder(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap, const int *snap_steps,
                             const hadi_jumps *jumps, double *out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples; x.jumps = jumps;
    CallOut o; o.pick = true; o.V_0 = V_0; o.prices = out;
    return solve_common(c, p, x, o);
}

int hadi_compute_base_prices_bates_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                                           const int *snap_steps, const hadi_jumps *jumps, double *out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples; x.jumps = jumps;
    CallOut o; o.rebuild_v = true; o.pick = true; o.V_0 = V_0; o.prices = out;
    return solve_common(c, p, x, o);
}

int hadi_compute_jacobian_bates_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, double eps, const hadi_samples *samples, int n_snap,
                                        const int *snap_steps, const hadi_jumps *jumps, int n_par, double *J, double *base) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (c && !jumps) return fail(c, HADI_ERR_INVALID, "jump description missing");
    if (c && n_par != 5 && n_par != 8) return fail(c, HADI_ERR_INVALID, "n_par must be 5 or 8 (is %d)", n_par);
    if (c && (n_snap < 1 || !snap_steps)) return fail(c, HADI_ERR_INVALID, "need 1 <= n_snap <= N snapshot steps");
    CallExtras x; x.ladder = true; x.n_snap = n_snap; x.snap_steps = snap_steps; x.sampled = true; x.samples = samples; x.jumps = jumps;
    if (n_par == 8) { x.jump_cols = true; x.jump_eps = eps; }
    CallOut o; o.V_0 = V_0; o.eps = eps; o.J = J; o.base_prices = base;
    return jacobian_common(c, p, x, o);
}

HADI_VARIANT_WRAPPERS(american, HADI_AM)
HADI_VARIANT_WRAPPERS(dividends, HADI_DIV)
HADI_VARIANT_WRAPPERS(american_dividends, HADI_AM_DIV)

// ---- Levenberg-Marquardt normal equations (jacobian_computation.cpp:20-195) ---------------------------
}  // extern "C"

namespace {
// [J^T J row-major NP^2][J^T r NP][sum r^2] of n rows of NP columns.
template <int NP>
void lm_partials_host(int n, const double *J, const double *r, double *out) {
    for (int k = 0; k < hadi_lm_doubles(NP); k++) out[k] = 0.0;
    for (int i = 0; i < NP; i++)
        for (int j = 0; j < NP; j++) {
            double s = 0.0;
            for (int k = 0; k < n; k++) s += J[(size_t)k * NP + i] * J[(size_t)k * NP + j];
            out[i * NP + j] = s;
        }
    for (int i = 0; i < NP; i++) {
        double s = 0.0;
        for (int k = 0; k < n; k++) s += J[(size_t)k * NP + i] * r[k];
        out[NP * NP + i] = s;
    }
    double s2 = 0.0;
    for (int k = 0; k < n; k++) s2 += r[k] * r[k];
    out[NP * NP + NP] = s2;
}

// delta = (J^T J with diagonal * (1 + lambda))^-1 J^T r by NP x NP partial-pivot elimination.
template <int NP>
void lm_solve_host(const double *part, double lambda, double *delta) {
    double A[NP * NP], b[NP];
    for (int i = 0; i < NP * NP; i++) A[i] = part[i];
    for (int i = 0; i < NP; i++) {
        A[i * NP + i] *= (1.0 + lambda);  // jacobian_computation.cpp:136-138
        b[i] = part[NP * NP + i];
    }
    for (int k = 0; k < NP; k++) {  // partial-pivot elimination, jacobian_computation.cpp:44-83
        int piv = k;
        double best = std::fabs(A[k * NP + k]);
        for (int r = k + 1; r < NP; r++)
            if (std::fabs(A[r * NP + k]) > best) { best = std::fabs(A[r * NP + k]); piv = r; }
        if (piv != k) {
            for (int col = 0; col < NP; col++) std::swap(A[k * NP + col], A[piv * NP + col]);
            std::swap(b[k], b[piv]);
        }
        const double pv = A[k * NP + k];
        for (int col = k + 1; col < NP; col++) A[k * NP + col] /= pv;
        b[k] /= pv;
        A[k * NP + k] = 1.0;
        for (int i = k + 1; i < NP; i++) {
            const double f = A[i * NP + k];
            for (int col = k + 1; col < NP; col++) A[i * NP + col] -= f * A[k * NP + col];
            b[i] -= f * b[k];
            A[i * NP + k] = 0.0;
        }
    }
    for (int k = NP - 1; k >= 0; k--) {
        double v = b[k];
        for (int col = k + 1; col < NP; col++) v -= A[k * NP + col] * b[col];
        b[k] = v;
    }
    for (int i = 0; i < NP; i++) delta[i] = b[i];
}

// f.template operator()<NP>() for the width n_par = 1 .. 8 (the caller has checked it).
template <class F>
void for_width(int n_par, F f) {
    switch (n_par) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}
}  // namespace

extern "C" {

int hadi_lm_partials_n(int n, int n_par, const double *J, const double *r, double *out) {
    if (n_par < 1 || n_par > HADI_LM_MAX_PAR || n < 0 || !out || (n > 0 && (!J || !r))) return HADI_ERR_INVALID;
    for_width(n_par, [&](auto w) { lm_partials_host<decltype(w)::value>(n, J, r, out); });
    return HADI_OK;
}

int hadi_lm_partials(int n, const double *J, const double *r, double *out) { return hadi_lm_partials_n(n, 5, J, r, out); }

int hadi_lm_partials_device_n(hadi_ctx *ctx, int n, int n_par, const double *J, const double *model_prices, const double *market_prices,
                              double *partials) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return HADI_ERR_INVALID;
    if (n_par < 1 || n_par > HADI_LM_MAX_PAR) return fail(c, HADI_ERR_INVALID, "n_par = %d outside 1..%d", n_par, HADI_LM_MAX_PAR);
    if (n < 0 || !partials || (n > 0 && (!J || !model_prices || !market_prices))) return fail(c, HADI_ERR_INVALID, "bad arguments");
    DeviceGuard guard(c->device);
    const size_t nd = (size_t)hadi_lm_doubles(n_par);
    int rc = ensure(c, c->lm31, (size_t)hadi_lm_doubles(HADI_LM_MAX_PAR) * sizeof(double));
    if (rc) return rc;
    if (n_par == 5)  // (the kernel of hadi_lm_partials_device, under its own name)
        hipLaunchKernelGGL(hadi_lm_partials_kernel, dim3(1), dim3(256), (size_t)21 * 256 * sizeof(double), c->stream, n, J, model_prices,
                           market_prices, ptr<double>(c->lm31));
    else
        hipLaunchKernelGGL(hadi_lm_partials_n_kernel, dim3(1), dim3(256), (size_t)hadi_lm_sums(n_par) * 256 * sizeof(double), c->stream, n_par,
                           n, J, model_prices, market_prices, ptr<double>(c->lm31));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(partials, c->lm31.p, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HADI_OK;
}

int hadi_lm_partials_device(hadi_ctx *ctx, int n, const double *J, const double *model_prices, const double *market_prices,
                            double *partial31) {
    return hadi_lm_partials_device_n(ctx, n, 5, J, model_prices, market_prices, partial31);
}

int hadi_lm_solve_n(int n_par, const double *partials, double lambda, double *delta) {
    if (n_par < 1 || n_par > HADI_LM_MAX_PAR || !partials || !delta) return HADI_ERR_INVALID;
    for_width(n_par, [&](auto w) { lm_solve_host<decltype(w)::value>(partials, lambda, delta); });
    return HADI_OK;
}

int hadi_lm_solve(const double *partial31, double lambda, double *delta5) { return hadi_lm_solve_n(5, partial31, lambda, delta5); }

int hadi_compute_parameter_update(int n, const double *J, const double *r, double lambda, double *delta5) {
    double part[31];
    int rc = hadi_lm_partials(n, J, r, part);
    if (rc) return rc;
    return hadi_lm_solve(part, lambda, delta5);
}

}  // extern "C"
