/*
 * hadi.h -- C ABI of libhadi: the MI355X-native batched Heston Douglas-ADI time stepper.
 *
 * Drop-in boundary for the hot path of BCW-dot/PDE-based-Heston-Solver-GPU-accelerated.
 * The reference has no FFI: its hot path is reached through the host-callable batched
 * launchers listed below (Kokkos templates).  Each entry point here takes, as flat arrays,
 * exactly the data those launchers take as Kokkos Views / struct arrays
 * (GridViews: grid_pod.hpp:8-15; DO_Workspace.U: DO_solver_workspace.hpp:7; U_0; dividend
 * views; model / market / numerics scalars), so a maintainer can bind it from the reference
 * host code with `view.data()` pointers -- see INTEGRATION.md.
 *
 *   hadi_DO_timestepping            <- device_DO_timestepping{,_american,_dividend,_american_dividend}
 *                                      (src/device_solver.hpp:194-266, 274-374, 382-641, 650-942)
 *                                      + Device_BoundaryConditions::initialize (hes_boundary_kernels.hpp:41-75)
 *                                      + Device_A{0,1,2}::build_matrix (hes_a0_kernels.hpp:30,
 *                                        hes_a1_kernels.hpp:51, hes_a2_shuffled_kernels.hpp:103)
 *                                      with scheme = HADI_SCHEME_CRAIG_SNEYD: CS_scheme_shuffled (src/solver.hpp:781-907)
 *   hadi_parallel_DO_solve          <- parallel_DO_solve (src/device_solver.hpp:52-185)
 *   hadi_compute_base_prices[_*]    <- compute_base_prices{,_american,_dividends,_american_dividends}
 *                                      (src/jacobian_computation.cpp:368, 629, 922, 1232)
 *   hadi_compute_jacobian[_*]       <- compute_jacobian{,_american,_dividends,_american_dividends}
 *                                      (src/jacobian_computation.cpp:204, 457, 726, 1031)
 *   hadi_compute_parameter_update   <- compute_parameter_update_on_device + solve_5x5_device
 *                                      (src/jacobian_computation.cpp:20-195)
 *   hadi_compute_greeks             <- no counterpart: delta, gamma, variance sensitivities, theta and the spot ladder of the
 *                                      v-row of V_0, from the state the sweep leaves on the device
 *   hadi_maturity_ladder, hadi_compute_{base_prices,jacobian}_ladder <- no counterpart: the price node after chosen steps of ONE sweep
 *                                      (a whole maturity ladder per strike on a shared delta_t)
 *   hadi_sample_ladder, hadi_compute_{base_prices,jacobian}_samples <- no counterpart: the ladder with the state of row V_0
 *                                      evaluated at arbitrary spots (4-point interpolants) on the device, inside the time loop
 *   hadi_bermudan_timestepping, hadi_compute_{base_prices,jacobian}_bermudan <- no counterpart: the European sweep with exercise
 *                                      on chosen steps (U <- max(U, payoff) at their end)
 *   hadi_barrier_timestepping, hadi_compute_{base_prices,jacobian}_barrier <- no counterpart: the European sweep with a knock-out
 *                                      on chosen monitoring steps (U <- rebate at or beyond a barrier, at their end)
 *   hadi_bates_timestepping, hadi_compute_{base_prices,jacobian}_bates, hadi_compute_jacobian_bates_jumps
 *                                   <- no counterpart: the European sweep under the Bates model
 *                                      (lognormal jumps as a dense sub-step U <- U + lambda dt G U at the end of every step)
 *   hadi_make_grid / hadi_rebuild_variance <- Grid::Grid (src/grid.cpp:16-61),
 *                                      GridViews::rebuild_variance_views (src/grid_pod.hpp:25-73)
 *
 * Conventions
 *   - All arithmetic is IEEE fp64.  Logical layout of every [n][m] field is the reference's:
 *     idx = i + j*(m1+1), i = s-index (fastest), j = v-index, m = (m1+1)(m2+1)
 *     (src/device_solver.cpp:713).  The library keeps its own internal HBM layout.
 *   - Array arguments live in the memory space named by hadi_problem.memspace
 *     (HADI_MEM_DEVICE: device pointers, data already resident in HBM; HADI_MEM_HOST: host
 *     pointers, the library stages them).  Scalars, per-instance parameter overrides and the
 *     dividend schedule are always host memory.  Outputs (base_prices, J) follow memspace.
 *   - Every call is synchronous on the handle's stream (the reference fences before returning:
 *     device_solver.hpp:184, jacobian_computation.cpp:363,447).  A handle is not thread-safe.
 *   - Return value: HADI_OK or an error code; hadi_last_error() gives the message.  The
 *     reference has `void` returns and silently reads index -1 when S_0 is not a grid node
 *     (jacobian_computation.cpp:275-288); here that is HADI_ERR_NOT_ON_GRID.
 *   - There is no CPU fallback: without a usable gfx950 device hadi_create fails.
 */
#ifndef HADI_H
#define HADI_H

#ifdef __cplusplus
extern "C" {
#endif

#define HADI_VERSION_MAJOR 0
#define HADI_VERSION_MINOR 2

typedef struct hadi_ctx hadi_ctx;

enum hadi_status {
    HADI_OK = 0,
    HADI_ERR_INVALID = 1,      /* bad argument (NULL, sizes, variant) */
    HADI_ERR_UNSUPPORTED = 2,  /* grid shape outside what the kernels cover */
    HADI_ERR_HIP = 3,          /* a HIP runtime call failed */
    HADI_ERR_NOT_ON_GRID = 4,  /* S_0 is not a node of some instance's s-grid (hadi_compute_greeks: or V_0 of its v-grid) */
    HADI_ERR_NO_DEVICE = 5,    /* no usable GPU: the product has no CPU path */
    HADI_ERR_ALLOC = 6,
    HADI_ERR_INTERNAL = 7      /* a kernel reported a failure through the handle's device error word (e.g. the bounded
                                  rendezvous of a two-wavefront row ran out of polls): the outputs of the call are invalid */
};

enum hadi_variant { HADI_EU = 0, HADI_AM = 1, HADI_DIV = 2, HADI_AM_DIV = 3 };
enum hadi_memspace { HADI_MEM_HOST = 0, HADI_MEM_DEVICE = 1 };
/* Splitting scheme.  The reference's device path is Douglas only (src/device_solver.hpp:194-266); Craig-Sneyd
 * exists in its host family (CS_scheme_shuffled, src/solver.hpp:781-907, European) and is offered here on the
 * device for the European variant.  Modified Craig-Sneyd and Hundsdorfer-Verwer (in 't Hout & Foulon) are second order
 * for every theta (Douglas is first order with the mixed-derivative term); the usual choices are theta = 1/3 for MCS and
 * theta = 1/2 + sqrt(3)/6 for HV.  MCS at theta = 1/2 is Craig-Sneyd.  All three predictor-corrector schemes: European
 * variant, call boundary data, fp64 state, m1 <= 1024 and m2 <= 527 (HADI_ERR_UNSUPPORTED otherwise); MCS and HV also
 * need theta > 0.  Grids that fit in LDS (m1 <= 128, m2 <= 32) run the whole time loop of such a sweep in one launch, one
 * wavefront per instance (hadi_small_sch_kernel; tuning key "small_sch" says when). */
enum hadi_scheme { HADI_SCHEME_DOUGLAS = 0, HADI_SCHEME_CRAIG_SNEYD = 1, HADI_SCHEME_MCS = 2, HADI_SCHEME_HV = 3 };
/* Precision of the state arrays BETWEEN the two directional passes.  FP64 is what the reference computes in.  FP32
 * ("mixed-precision fp32 ADI sweep with fp64 tridiag pivots", BASELINE.json config 5): U and the A2 right-hand side are
 * stored as fp32 in HBM (half the traffic: 16 B per point-step), every operator, pivot and line solve is still
 * evaluated in fp64 in registers.  European Douglas sweeps (HADI_EU, HADI_DIV) only; the caller's arrays stay fp64.
 * Not a reference feature: parity is against the oracle run with the same two roundings per step (tests).  Each rounding
 * perturbs the state by 2^-24 relative and the perturbations add up like a random walk over the steps: against the
 * fp64 sweep the price moves by 1e-7 .. 1.5e-5 (erratic in N: one realisation of the walk per run; 1.5e-5 at
 * 1024x512x2000) and the field by up to 1.4e-5 of max|U| at N = 2000 (increments below half an fp32 ulp are absorbed by
 * the rounding) -- a throughput mode for users who accept that; it does NOT guarantee a 1e-6 price tolerance. */
enum hadi_state_precision { HADI_STATE_FP64 = 0, HADI_STATE_FP32 = 1 };
/* Boundary data of the option type.  HADI_CALL is the reference's only boundary class (call-specific,
 * src/BoundaryConditions.hpp:7-12, hes_boundary_kernels.hpp:41-75).  HADI_PUT is NOT a reference feature (README.md:26
 * claims puts, no code exists): the same operators with the put's boundary data --
 *   s = s_max:  du/ds = 0             -> b1 == 0                  (call: du/ds = e^{-r_f t} -> b1 = (r_d - r_f) s_max E)
 *   v = v_max:  u = K e^{-r_d t}      -> b2 = -1/2 r_d K on the last v-row, time factor e^{-r_d dt n}
 *                                                                  (call: u = s e^{-r_f t} -> b2 = -1/2 r_d s_i E)
 *   s = 0:      u = K e^{-r_d t}      -> the i = 0 row of A1 carries the reaction term -1/2 r_d like every other row
 *                                        (the call leaves that row empty, hes_a1_kernels.hpp:56-61: its value stays 0)
 *   v = 0 and the two top v-rows: the PDE rows / empty rows of A2 exactly as for the call.
 * Needs hadi_problem.strike_i.  Validated by put-call parity against the call path and the semi-analytic Heston price. */
enum hadi_option_type { HADI_CALL = 0, HADI_PUT = 1 };

/* Columns of hadi_compute_greeks' outputs (one row of 8 per node). */
enum hadi_greek {
    HADI_GREEK_PRICE = 0,   /* U(i, j0) */
    HADI_GREEK_DELTA = 1,   /* dU/ds */
    HADI_GREEK_GAMMA = 2,   /* d2U/ds2 */
    HADI_GREEK_DV = 3,      /* dU/dv, the sensitivity to the spot variance (Black-Scholes-style vega = dv * 2 sqrt(v): the caller's) */
    HADI_GREEK_DVV = 4,     /* d2U/dv2 */
    HADI_GREEK_DSV = 5,     /* d2U/ds dv */
    HADI_GREEK_THETA = 6,   /* calendar-time derivative per year */
    HADI_GREEK_LAMBDA = 7,  /* lambda_bar of the American variants (> 0: exercise region), 0 otherwise */
    HADI_N_GREEKS = 8
};

/* One batch of independent option instances = one league of teams in the reference
 * (TeamPolicy(nInstances, AUTO), device_solver.hpp:83-88). */
typedef struct hadi_problem {
    int n_instances;
    int m1, m2;            /* grid intervals: (m1+1) s-nodes, (m2+1) v-nodes */
    int variant;           /* enum hadi_variant */
    int memspace;          /* enum hadi_memspace, applies to the array fields below */

    /* time discretisation (shared); N_i / delta_t_i override per instance (multi-maturity,
     * heston_calibration.cpp:2165-2171), host arrays of length n_instances or NULL */
    int N;
    double delta_t;
    double theta;
    const int *N_i;
    const double *delta_t_i;

    /* market + Heston parameters (shared across the batch in the reference,
     * jacobian_computation.cpp:206-208); *_i override per instance (host arrays) or NULL */
    double r_d, r_f;
    double rho, sigma, kappa, eta;
    const double *rho_i, *sigma_i, *kappa_i, *eta_i;

    /* GridViews, one row per instance (grid_pod.hpp:9-15) */
    const double *vec_s;   /* [n][m1+1] */
    const double *vec_v;   /* [n][m2+1] */
    const double *delta_s; /* [n][m1]   */
    const double *delta_v; /* [n][m2]   */

    /* discrete dividends, shared (device_solver.hpp:409-413); host arrays.
     * Dating is the reference's rule (device_solver.hpp:424-517), mirrored as it stands: the dates are consumed in ARRAY
     * order by one running index.  At the start of step n = 1..N the dividend under the index is paid if
     * n*delta_t <= date < (n+1)*delta_t, both products evaluated in fp64 (12 * 0.05 = 0.6000000000000001 > 0.6 decides the
     * step); after the step the index advances by one if n*delta_t > date -- at most once per step.  Hence: a date earlier
     * than delta_t is never paid; of two dates inside one step interval the second is skipped; a cluster of dates makes the
     * index lag behind later ones, which are then skipped too; unsorted dates are not sorted; and two paying steps are
     * never adjacent (the index leaves a paid date one step later and sees the next date one step after that), so a
     * schedule with a date in every step interval pays the first one only.  A date in [N*delta_t, (N+1)*delta_t) is paid at
     * the start of the last step, later ones never.
     * The jump U(s) <- U(s (1 - percentage) - amount) interpolates linearly between the two nodes around the ex-dividend
     * spot; at or below 0 a call takes 0 and a put its value at node 0; and when NO node lies above the ex-dividend spot, or
     * node 0 already does, it takes node 0's value -- so a zero dividend is not the identity at s_max, and neither is a
     * negative one (the reference's idx == 0 branch). */
    int num_dividends;
    const double *dividend_dates, *dividend_amounts, *dividend_percentages;

    /* DO_Workspace.U: in = initial condition, out = solution at T.  [n][m] */
    double *U;
    /* payoff for the American projection (U_0_i, device_solver.hpp:304); [n][m].
     * NULL = use the initial U. */
    const double *U_0;
    /* optional output: lambda_bar at T (DO_solver_workspace.hpp:22); [n][m] or NULL */
    double *lambda_bar;
    /* enum hadi_scheme; 0 (Douglas) is what every reference launcher runs */
    int scheme;
    /* enum hadi_state_precision; 0 (fp64) is what every reference launcher runs */
    int state_precision;
    /* enum hadi_option_type; 0 (call boundary data) is what every reference launcher runs */
    int option_type;
    /* strikes, host array [n]; required for HADI_PUT (boundary value K e^{-r_d t}), ignored for HADI_CALL */
    const double *strike_i;
    /* hadi_compute_base_prices* / hadi_compute_jacobian* only: per-instance V_0 (host array [n]) overriding the
     * scalar argument -- every instance's v-grid is rebuilt on the device for its own V_0, as every team of the
     * reference does in-kernel (GridViews::rebuild_variance_views, src/grid_pod.hpp:25-73).  NULL = the scalar V_0. */
    const double *V_0_i;
} hadi_problem;

/* Timing of the last sweep on this handle, measured with HIP events on the handle's
 * stream.  Kernel sums are only filled when profiling was enabled with hadi_set_profiling. */
typedef struct hadi_timing {
    double setup_ms;        /* staging + operator/boundary setup + layout pack */
    double sweep_ms;        /* the N-step time loop only */
    double finish_ms;       /* unpack + price pick */
    double pass_a_ms;       /* sum over launches of the row-pass kernel   (profiling only) */
    double pass_b_ms;       /* sum over launches of the column-pass kernel (profiling only) */
    long long pass_a_launches, pass_b_launches;
    long long point_steps;  /* sum over instances of (m1+1)(m2+1)*N_i */
} hadi_timing;

/* ---- handle ----------------------------------------------------------------------------- */
int hadi_create(hadi_ctx **out, int device_id);
int hadi_destroy(hadi_ctx *ctx);
const char *hadi_last_error(const hadi_ctx *ctx);
const char *hadi_status_string(int status);
int hadi_version(void);
int hadi_set_profiling(hadi_ctx *ctx, int enabled);
int hadi_get_timing(const hadi_ctx *ctx, hadi_timing *out);
/* Execution-path switches (results agree to round-off; the library reads NO environment variables):
 *   "small_grid"  LDS-resident one-launch path for grids that fit in LDS (default 1)
 *   "small_seq"   ... European / dividend sweeps of such grids on the one-wavefront-per-instance kernel that solves the
 *                 lines sequentially, one per lane: -1 automatic (default: batches of more instances than CUs), 0 never
 *                 (the block-per-instance kernel, which the American sweeps always use), 1 always
 *   "small_sch"   Craig-Sneyd / MCS / HV sweeps of grids with m1 <= 128 and m2 <= 32 on the LDS-resident kernel that runs the
 *                 whole time loop in one launch, one wavefront per instance (hadi_small_sch_kernel; needs "small_grid", no
 *                 profiling): -1 automatic (default), 0 never (the streaming kernels), 1 wherever the grid is admitted.
 *                 Automatic: batches of more instances than CUs, on grids of which a CU's 160 KiB of LDS hold at least three
 *                 instances (four fields of (m2 + 1) x ((m1 + 3) | 1) doubles each plus ~4 KB of tables: 50x25 yes, 64x32 and
 *                 100x30 no), unless the caller pinned the streaming geometry ("strip", "row_tile", "col_groups",
 *                 "strip_blocks", or "cs_strips" = 0).  Measured on 50x25, 257 ... 3000 instances: 2.0 - 2.6x the streaming
 *                 kernels; on 100x30 x500 (one instance per CU) 0.79x, which is why such grids stay streaming
 *                 (profiles/r08_small_sch_ab.txt)
 *   "graph"       hipGraph replay of the time loop for small batches (default 1).  The handle caches up to 8 captured loops,
 *                 keyed by everything their nodes bake in: the launch geometry of every sub-batch, the scheme, variant and
 *                 precision, the steps that carry a dividend, the snapshot steps of a ladder call (and the sample count of a sample call: its taps are data, located again on every call), the exercise steps of a Bermudan call, the monitoring steps of a barrier call, and every device address the loop uses (the library's buffers --
 *                 rs_tab and the fp64 packed U of an fp32-state sweep among them -- and the caller's s-grid).  Whenever a call
 *                 frees a buffer to grow it, the whole cache is dropped first, so a replay never touches freed memory.
 *                 Read-only counters, cumulative over the handle's life (hadi_get_tuning only; hadi_set_tuning returns
 *                 HADI_ERR_INVALID): "graph_captures" loops captured, "graph_replays" loops replayed from the cache,
 *                 "graph_drops" cache entries destroyed because a buffer was freed, "graph_evictions" entries evicted as least
 *                 recently used (counted apart from the drops)
 *   "american_p"  American sweeps keep P = U_bar - dt*lambda_bar in place of U and no lambda_bar array whenever every
 *                 payoff of the batch depends on s only (default 1; 0 = always the explicit (U, lambda_bar) pair)
 *   "strip"       strip row pass: -1 automatic (default), 0 never, 1 whenever the geometry allows it
 *   "row_tile"    shared-ring row pass: v-rows per block tile (0 = automatic)
 *   "strip_blocks" strip row pass: blocks per instance (0 = automatic)
 *   "model_strip_row_ns", "model_ring_row_ps", "model_ring_fixed_ns", "model_pstrip_row_ns", "model_pring_row_ps",
 *   "model_pring_fixed_ns"  constants of the cost model that decides between strips and the shared ring at 8 nodes per lane
 *                 (hadi_plan.h; defaults 2800 / 2330 / 12000 and, for two wavefronts per row, 3250 / 4300 / 15000: measured on
 *                 one MI355X, the boxes of a pool differ by +-3 % on the kernels they model)
 *   "pair_strips" strip row pass at 4 nodes per lane (128 < m1 <= 256): two strips per wavefront on the 8-nodes-per-lane
 *                 arithmetic (hadi_pass_a_pairs): -1 automatic (default: where the launch still has two blocks per CU and the
 *                 strips keep 16 rows, e.g. 512 instances of 256x128), 0 never, 1 wherever the strips run
 *   "col_groups"  column pass: blocks per instance (0 = automatic)
 *   "small_waves" small-grid kernel: wavefronts per instance, 4 or 8 (0 = automatic)
 *   "small_pairs" LDS-resident European / dividend sweeps: two instances per wavefront (hadi_small_seq2_kernel; grids of at most
 *                 32 v-rows): -1 automatic (default: batches of more than 2 and at most 4.5 instances per CU, where it is 14 - 20 %
 *                 faster), 0 never, 1 whenever possible
 *   "sub_batch"   batches of several rounds of one instance per CU on grids whose round exceeds the 256 MB memory-side
 *                 cache run sub-batch by sub-batch through the time loop (default 1; instances are independent)
 *   "streams"     0 (default) automatic, 1 one stream, 2 two streams.  On two streams the two halves of a Douglas batch run their
 *                 time loops side by side (fork / join by events inside the call; per-launch profiling switches it off).
 *                 Same kernels, same results.  It pays where the row pass of the whole batch leaves a partial round of CUs
 *                 idle -- 512x256: 160 instances +7 %, 192: +16 %, 24..32: +14..22 % -- and costs 2..12 % where the launches
 *                 fill whole rounds (64, 128, 256, 512 instances): the automatic choice cuts the batch (or the remainder
 *                 behind its full rounds of one instance per CU) in two exactly when the plan's row pass leaves 4 % or more
 *                 of its CU-rounds idle (hadi_plan_row_idle) -- a function of the grid shape and the batch size alone.
 *                 With 2 the sub-batches of a large batch alternate between the streams -- and so they do in the automatic mode
 *                 when a batch is several sub-batches of strip launches (measured never slower, +3 .. +6 % with a remainder behind
 *                 one full round); DESIGN.md sections 4.2, 7
 *   "col_prefetch" 0 (default) / 1: European sweeps of 9 .. 16 chunks (264 <= m2 <= 527) on hadi_pass_b2 -- part of the next column
 *                 tile prefetched into LDS by LDS-DMA -- instead of hadi_pass_b1; "tile_interleave" 0 (default) / 1: the blocks of
 *                 an instance walk their column tiles interleaved.  Both measured within +-2 % (profiles/r04_colpass_ab.txt);
 *                 same bits as the default path
 *   "cs_strips"   1 (default) / 0: the predictor / corrector row passes of a Craig-Sneyd sweep on the barrier-free strips wherever
 *                 the plan picks strips (0: on the shared ring, the path of rounds 2 - 3; same fields to round-off)
 *   "graph_max_melems" hipGraph replay of the time loop for batches of up to this many Mi state elements (default 8; larger
 *                 batches are not launch-bound: measured equal)
 *   "jump_share"  1 (default) / 0: hadi_compute_jacobian_bates_jumps with per-instance matrices -- the groups 0 .. 6 of an instance
 *                 share one staged strip of its matrix (0: every block stages the strip for one instance); same bits
 *   "device_vgrid" v-grids of compute_base_prices / compute_jacobian rebuilt per instance on the device (default 1;
 *                 0 = built once on the host with glibc sinh/asinh and broadcast -- bit-identical to the reference's
 *                 host-side Grid, needs one shared V_0)
 *   "team_launch" instance-resident execution of batches of up to 8 large European instances, with or without discrete dividends
 *                 (128 < m1 <= 512, m2 <= 263):
 *                 the whole time loop in ONE launch, every instance kept in the L2 of one XCD by a team of 32 blocks
 *                 (hadi_team_kernel): -1 automatic (default), 0 never, 1 whenever the shape allows it.  If the team
 *                 protocol fails (it is bounded everywhere) the batch is solved again on the two-launches-per-step path
 *                 and the automatic choice stays away from it for the rest of the handle's life (get: -2)
 *   "resident_sweep" both passes of every Douglas step in ONE launch per sub-batch, one 512-thread block per instance running
 *                 its whole time loop (hadi_sweep_resident<8>: the row phase is the body of hadi_pass_a_strip<8,EU>, the column
 *                 phase the hadi_pb_* functions of hadi_pass_b<8,EU>, a workgroup barrier between them): -1 automatic
 *                 (default), 0 never, 1 wherever eligible.  Eligible: European Douglas sweeps with the fp64 state,
 *                 256 < m1 <= 512, m2 <= 263, theta > 0, r_d != r_f, a sub-batch whose strip row pass is one block per
 *                 instance in one round of CUs with less than 4 % of them idle (512x256: 246 .. 256 instances per round;
 *                 a remainder sub-batch stays streaming).  Under -1 a caller who pins the streaming geometry ("strip",
 *                 "row_tile", "col_groups", "strip_blocks") gets the streaming kernels, and so does any "debug_fault" hook.
 *                 Per-launch profiling
 *                 (hadi_set_profiling) needs a kernel per pass: with it on, the sweep runs on the streaming kernels.  Same
 *                 bits as the streaming path; 512x256 x256 x1000 steps 212.3 -> 201.2 ms
 *   "debug_fault" TEST HOOK, 0 in production: 1 = the high half of every two-wavefront row (m1 > 512) withholds its
 *                 rendezvous token on v-row 1, so that the partner's bounded poll runs out (~0.2 s) -- the call must then
 *                 return HADI_ERR_INTERNAL instead of a field solved with stale exchange values; 128 = one block of every
 *                 team of an instance-resident launch deserts before the first team barrier -- the launch must time out,
 *                 and the call must still return the right field (from the two-launches-per-step path); 16 / 32 / 64 =
 *                 timing diagnostics of that launch (row phase / column phase / barriers skipped: results are wrong); 256 / 512 =
 *                 timing diagnostics of the column pass (tiles loaded and stored but not solved / solved without the reduced
 *                 system: results are wrong; tools/colpass_ab.py) */
int hadi_set_tuning(hadi_ctx *ctx, const char *key, int value);
int hadi_get_tuning(const hadi_ctx *ctx, const char *key, int *value);
/* Device the handle runs on: name, CU count, gcn arch string (for bench reports). */
int hadi_device_info(const hadi_ctx *ctx, char *name, int name_len, int *compute_units, char *arch, int arch_len);
/* Which kernels the last sweep on this handle ran (kernel names and tile geometry), for bench reports and profiles. */
int hadi_describe_last_sweep(const hadi_ctx *ctx, char *buf, int len);
/* Opaque hipStream_t of the handle (void*), so callers can order their own work after it. */
void *hadi_stream(hadi_ctx *ctx);
/* Input ordering (HADI_MEM_DEVICE).  The handle runs on its own non-blocking stream, which does not wait for the
 * caller's streams: work the caller enqueued on `producer_stream` (a hipStream_t; NULL = the legacy default stream)
 * that writes arrays of the next hadi_* call must be ordered before it with this call (an event is recorded on
 * `producer_stream` and the handle's stream waits for it; nothing blocks on the host), or the caller must synchronise
 * that stream itself.  The reference gets the same guarantee from deep_copy + Kokkos::fence (device_solver.cpp:718-726).
 * Outputs need no such call: every hadi_* entry point returns after its results are complete. */
int hadi_wait_stream(hadi_ctx *ctx, void *producer_stream);

/* ---- grids (host code, no GPU needed) ------------------------------------------------------ */
int hadi_make_grid(int m1, double S, double S_0, double K, double c,
                   int m2, double V, double V_0, double d,
                   double *vec_s, double *vec_v, double *delta_s, double *delta_v);
int hadi_rebuild_variance(int m2, double V_0_new, double V, double d, double *vec_v, double *delta_v);
int hadi_find_s_index(int m1, const double *vec_s, double S_0);  /* -1 if not a node */
int hadi_find_v_index(int m2, const double *vec_v, double V_0);  /* 0 if not a node (grid_pod.hpp:76-87) */

/* ---- the hot path -------------------------------------------------------------------------- */
int hadi_DO_timestepping(hadi_ctx *ctx, const hadi_problem *p);

int hadi_parallel_DO_solve(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                           double *base_prices /* [n] */);

/* Greeks at (S_0, V_0) and, optionally, the spot ladder of the v-row of V_0 -- NOT a reference feature (the reference returns
 * prices and forward-difference parameter sensitivities only).  The sweep of hadi_DO_timestepping (p is read exactly as that
 * entry point reads it: the caller's four grid arrays, variant, dividends, scheme, option type and strikes, per-instance
 * parameters and (N_i, dt_i), U_0, the initial condition p->U) followed by ONE small kernel on the state and the operator
 * tables the sweep left in HBM (hadi_greeks_kernel).  p->U and p->lambda_bar are NOT written and no field leaves the device:
 * the results are n*8 doubles (and n*(m1+1)*8 with the ladder).
 *   greeks [n][8]        the row of the node i0 = first s-node with |s_i - S_0| < 1e-10, on the v-row j0 = first v-node with
 *                        |v_j - V_0| < 1e-10; columns: enum hadi_greek
 *   ladder [n][m1+1][8]  the same 8 columns for every s-node of row j0, or NULL (ladder[k][i0] == greeks[k] bit for bit)
 * Both follow p->memspace.  Stencils: three-point first and second derivatives on the non-uniform axes -- interior nodes the
 * reference's beta / delta weights (coeff.hpp), end nodes its one-sided gamma (first node) / alpha (last node) weights; the
 * second derivative of an end node is its interior neighbour's (one parabola through the three nodes).  All are exact on
 * quadratics.  dsv is D1_v applied to the rows D1_s U(., j): inside the grid the 9-point product stencil of A0.
 * theta = -(A0 U + A1 U + A2 U + b e_N + lambda_bar_N)(i, j0): minus the explicit right-hand side F(t_N, U_N) of the scheme,
 * evaluated from the sweep's own operator tables and boundary vector, e_N = exp(bc_rate dt N), bc_rate = r_f (call data) or
 * -r_d (put data), with the instance's own parameters and (N, dt).  Two things to know about it:
 *   - it includes the reference's boundary-vector quirks: the call's b1 entry of v-row j sits at column m1 - j
 *     (hes_boundary_kernels.hpp:54-58), an INTERIOR node of the ladder -- on 256x128 with V_0 = 0.04 that is i = 217;
 *   - for American options it is the semi-discrete residual: accurate away from the free boundary, about 0 deep inside the
 *     exercise region, and O(1) off on the few nodes next to the boundary (on the oracle's field of a 100x50 American put its
 *     largest value over the exercised ladder nodes is 0.03 .. 0.4 for N = 100 .. 200 and up to 12 for N = 20, its median
 *     below 1e-6).  No backward difference of the last two time levels is formed.
 * Errors: everything hadi_DO_timestepping refuses, with the same status (p->V_0_i: HADI_ERR_INVALID); greeks == NULL:
 * HADI_ERR_INVALID; HADI_STATE_FP32: HADI_ERR_UNSUPPORTED (a gamma stencil on 512x256 has weight sums near 1e2: on a state
 * rounded to 24 bits it returns noise); S_0 off some instance's s-grid: HADI_ERR_NOT_ON_GRID, as the price pick.  V_0 off some
 * instance's v-grid is HADI_ERR_NOT_ON_GRID as well -- UNLIKE the price pick of hadi_parallel_DO_solve / hadi_compute_base_prices,
 * which mirrors the reference and silently reads v-row 0: a Greek taken on the wrong row is not returned silently.
 * Whenever the call returns an error, the contents of greeks and ladder are unspecified. */
int hadi_compute_greeks(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                        double *greeks /* [n][8] */, double *ladder /* [n][m1+1][8] or NULL */);

/* Maturity ladder -- NOT a reference feature.  A sweep of N steps passes through the solution of every shorter time to maturity
 * n dt; these three calls return the price node after each of the steps snap_steps[0 .. n_snap) of ONE sweep, where a call per
 * maturity would run sum(snap_steps) steps.  By definition snapshot q is what the same call with N = snap_steps[q] returns, bit for
 * bit on the same execution path: the dividend dating only looks backwards, the carry-over arrays of CS / MCS / HV come from earlier
 * steps and the boundary time factor depends on n dt only.  This is NOT the reference's multi-maturity convention (N_m = max(20,
 * int(20 T_m)), dt_m = T_m / N_m): a ladder shares one dt.  For the dividend variants the dates are read on the sweep's clock, as in
 * a single call: all maturities of the ladder share the one schedule.
 *   snap_steps  host array, strictly increasing, every entry in 1 .. p->N, 1 <= n_snap <= p->N; the last need not be N
 *   prices      [n][n_snap];  J [n][n_snap][5], base_prices [n][n_snap] (the 6n-group layout of hadi_compute_jacobian inside);
 *               all follow p->memspace
 * hadi_maturity_ladder reads p as hadi_compute_greeks does (the caller's four grids, variant, dividends, scheme, option type and
 * strikes, per-instance parameters, U_0, the initial p->U); hadi_compute_base_prices_ladder / hadi_compute_jacobian_ladder rebuild
 * the v-grid and honour V_0_i exactly as hadi_compute_base_prices / hadi_compute_jacobian do, the variant from p->variant.  p->U
 * and p->lambda_bar are not written.  delta_t_i is allowed (every instance its own ladder in time on the shared step indices).  The
 * node is the price pick's: first s-node within 1e-10 of S_0, v-row 0 if V_0 is off the v-grid; a small kernel locates it before
 * the sweep (hadi_locate_kernel).  The LDS-resident whole-loop kernels copy the node's value out inside their time loop; the
 * streaming kernels are followed by a hadi_snap_kernel on snapshot steps.  A ladder call runs American sweeps on the explicit
 * (U, lambda_bar) pair and never takes hadi_sweep_resident or hadi_team_kernel: those batches run the streaming kernels, as under profiling.
 * Errors: N_i != NULL, a bad snap_steps or a NULL output: HADI_ERR_INVALID; HADI_STATE_FP32: HADI_ERR_UNSUPPORTED; S_0 off some
 * instance's s-grid: HADI_ERR_NOT_ON_GRID; everything else the underlying entry point refuses keeps its status.  One more:
 * call boundary data with r_f != 0 is HADI_ERR_UNSUPPORTED -- the call's boundary vector carries exp(-r_f dt (N - 1))
 * (hes_boundary_kernels.hpp:56), so the tables depend on N and the intermediate states are not the shorter sweeps' results; puts
 * (whose boundary factor is exp(-r_d dt n)) and calls with r_f = 0 have the property exactly. */
int hadi_maturity_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_snap, const int *snap_steps,
                         double *prices /* [n][n_snap] */);
int hadi_compute_base_prices_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_snap, const int *snap_steps,
                                    double *prices /* [n][n_snap] */);
int hadi_compute_jacobian_ladder(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, int n_snap,
                                 const int *snap_steps, double *J /* [n][n_snap][5] */, double *base_prices /* [n][n_snap] */);

/* Sampled ladder -- NOT a reference feature.  The ladder returns one number per instance and snapshot: the node where S_0 sits.
 * These three calls evaluate the state of the same v-row at n_samp arbitrary spots instead, inside the time loop, on the device;
 * the field never leaves the GPU.  A sample call IS a ladder call: the same route and kernels, admitted and refused exactly where
 * hadi_maturity_ladder / hadi_compute_base_prices_ladder / hadi_compute_jacobian_ladder are (American sweeps on the explicit
 * pair, never the resident sweep or the team launch, HADI_STATE_FP32 and call data with r_f != 0: HADI_ERR_UNSUPPORTED, N_i:
 * HADI_ERR_INVALID; delta_t_i, V_0_i, puts, dividends and the predictor-corrector schemes are allowed); wherever the ladder copies
 * one node, a sample call evaluates n_samp interpolants.  snap_steps = {N} is the plain "sample at T" use.
 *
 * Definition of a sample.  For instance k the row is j0 by the ladder's rule: the first v-node within 1e-10 of V_0 (or V_0_i[k]),
 * row 0 if there is none.  With s_0 < .. < s_m1 the nodes of the instance's own vec_s and x the spot:
 *   node hit    if some |s_i - x| < 1e-10, the first such i is a single tap: the value is U(i, j0) bit for bit, times the scale.
 *               With scale 1 and x = S_0 this is exactly what hadi_maturity_ladder returns.
 *   off grid    if x is NaN, or x < s_0, or x > s_m1 beyond that tolerance, the entry is NaN and the call returns
 *               HADI_ERR_NOT_ON_GRID (the ladder's status for S_0 off the s-grid); the other entries are valid.
 *   interior    otherwise i is the largest index with s_i < x and the stencil starts at i0 = min(max(i - 1, 0), m1 - 3) (clamped at
 *               both ends).  w_a = prod_{b != a} (x - s_{i0+b}) / prod_{b != a} (s_{i0+a} - s_{i0+b}), a = 0..3, numerator and
 *               denominator each accumulated over increasing b, then one division.  The value is
 *               fma(w3, U3, fma(w2, U2, fma(w1, U1, w0 * U0))) with U_a = U(i0 + a, j0), then one multiplication by the scale.
 *   degenerate  a stencil with a zero interval (or m1 < 3) gives non-finite weights: the entry is NaN, the call returns
 *               HADI_ERR_INVALID (which takes precedence over an off-grid sample of the same call).
 * Cubic, because a linear interpolant adds Gamma ds^2 / 8, the same order as the scheme's own spatial error; the 4-point one does not.
 * For a Jacobian the six groups' samples are located on the groups' own rebuilt v-grids: the v0 column samples its own row.
 * Errors beyond the ladder's (which keep their status): a NULL struct, spots or output, n_samp outside 1..1024, rows other than 1
 * or n_instances, a non-finite scale: HADI_ERR_INVALID.  Outputs follow p->memspace; spots / scales / snap_steps are host arrays. */
typedef struct hadi_samples {
    int n_samp;            /* 1 .. 1024 samples per instance */
    const double *spots;   /* host [rows][n_samp]: spot x_q at which the state is evaluated */
    const double *scales;  /* host [rows][n_samp] or NULL (= 1): out = scale_q * U(x_q, V_0) */
    int rows;              /* 1 (one list for the batch) or n_instances */
} hadi_samples;
int hadi_sample_ladder(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                       const int *snap_steps, double *out /* [n][n_snap][n_samp] */);
int hadi_compute_base_prices_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                                     const int *snap_steps, double *out /* [n][n_snap][n_samp] */);
int hadi_compute_jacobian_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, double eps, const hadi_samples *samples,
                                  int n_snap, const int *snap_steps, double *J /* [n][n_snap][n_samp][5] */,
                                  double *base /* [n][n_snap][n_samp] */);

/* Bermudan options -- NOT a reference feature.  A Bermudan sweep is the European sweep of hadi_DO_timestepping (variant HADI_EU
 * or HADI_DIV) with one addition: after the last pass of every listed step n, every node of every instance that lists n takes
 * U <- max(U, payoff) -- all (m1+1)(m2+1) nodes, boundary rows and columns included.  The payoff is p->U_0, or the initial p->U
 * where U_0 is NULL.  Step n is time to maturity n delta_t_k on the instance's own clock; n = N_k is exercise at the valuation
 * date.  A dividend acts at the START of its step, exercise at the END; a step may carry both.  With a predictor-corrector scheme
 * the exercise follows the corrector's column pass.  lambda_bar is neither used nor written.
 *   ex_steps  host array [ex_rows][n_ex]; ex_rows is 1 (one schedule for the batch) or n_instances.  Each row is strictly
 *             increasing within 1 .. N_k and may end in zeros (an instance with fewer dates); with ex_rows == 1 every entry must be
 *             <= every instance's N_k.  n_ex == 0 is the plain European call: same route, same bits.
 * hadi_bermudan_timestepping reads and writes p exactly as hadi_DO_timestepping does (per-instance parameters, (N_i, delta_t_i), put
 * data with strike_i, dividends, scheme, memory space).  The two launchers rebuild the v-grid and honour V_0_i exactly as
 * hadi_compute_base_prices / hadi_compute_jacobian do, the variant from p->variant; the six groups of a Jacobian share their
 * instance's schedule.  The LDS-resident whole-loop kernels apply the exercise inside their time loop (the payoff read from its
 * packed global array on exercise steps only); the streaming kernels are followed by hadi_exercise_kernel on the steps that some
 * instance lists.  A Bermudan call never takes hadi_sweep_resident or hadi_team_kernel: those batches run the streaming kernels.
 * Errors: HADI_AM / HADI_AM_DIV or HADI_STATE_FP32: HADI_ERR_UNSUPPORTED; a bad schedule (an entry outside 1 .. N_k, not
 * increasing, a non-zero behind a zero), ex_rows other than 1 or n, n_ex < 0: HADI_ERR_INVALID; everything the underlying entry
 * point refuses keeps its status. */
int hadi_bermudan_timestepping(hadi_ctx *ctx, const hadi_problem *p, int n_ex, const int *ex_steps, int ex_rows);
int hadi_compute_base_prices_bermudan(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, int n_ex, const int *ex_steps,
                                      int ex_rows, double *base_prices);
int hadi_compute_jacobian_bermudan(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, int n_ex,
                                   const int *ex_steps, int ex_rows, double *J, double *base_prices);

/* Discretely monitored knock-out barrier options -- NOT a reference feature.  A barrier sweep is the sweep of hadi_DO_timestepping
 * (variant HADI_EU or HADI_DIV) with one addition: after the last pass of every listed monitoring step n, every node (i, j) of every
 * instance k that lists n is knocked if its spot node satisfies s_i <= lower_k or s_i >= upper_k -- touching knocks out; the
 * comparison is on the instance's own vec_s, in fp64 -- and a knocked node takes U <- rebate_k, in every v-row, boundary rows
 * included.  The rebate is paid at the knock-out: no discounting is applied.  Step n is time to maturity n delta_t_k on the
 * instance's own clock; n = N_k is the valuation date.  A dividend acts at the START of its step, the barrier at its END; a step may
 * carry both.  With a predictor-corrector scheme the knock-out follows the corrector's column pass.
 * MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's (the Dirichlet data at s_max and the v-edges are
 * those of the European call or put); between two monitoring dates the contract is alive everywhere.
 * The initial condition is the caller's: monitoring AT maturity is applied to the payoff by the caller.
 *   lower_i, upper_i, rebate_i  host arrays [n] or NULL.  NULL = no barrier on that side (-inf / +inf are allowed in the arrays and
 *             mean the same) / a rebate of 0.  An instance may have no live node at all.
 *   mon_steps host array [mon_rows][n_mon], the rules of ex_steps above: mon_rows is 1 or n_instances, each row strictly increasing
 *             within 1 .. N_k and zero-padded; with one shared row every entry must be <= every instance's N_k.  n_mon == 0 is
 *             the plain European call: same route, same bits.
 * hadi_barrier_timestepping reads and writes p exactly as hadi_bermudan_timestepping does; the two launchers rebuild the v-grid and
 * honour V_0_i as the Bermudan launchers do, and the six groups of a Jacobian share their instance's barrier, rebate and schedule.
 * The LDS-resident whole-loop kernels (hadi_small_sch_kernel among them) knock their field inside the time loop; the streaming
 * kernels are followed by hadi_knockout_kernel on the steps that some instance lists.  A barrier call never takes
 * hadi_sweep_resident or hadi_team_kernel.
 * Errors: HADI_AM / HADI_AM_DIV or HADI_STATE_FP32: HADI_ERR_UNSUPPORTED; a schedule that breaks the rules, a NULL barrier struct,
 * NaN in any array, lower_k >= upper_k, both arrays NULL with n_mon > 0, a non-finite rebate, a NULL output: HADI_ERR_INVALID;
 * everything the underlying entry point refuses keeps its status. */
typedef struct hadi_barrier {
    const double *lower_i, *upper_i, *rebate_i; /* host [n] or NULL */
    int n_mon;
    const int *mon_steps;
    int mon_rows; /* [mon_rows][n_mon], the rules of ex_steps */
} hadi_barrier;
int hadi_barrier_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_barrier *barrier);
int hadi_compute_base_prices_barrier(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_barrier *barrier,
                                     double *base_prices);
int hadi_compute_jacobian_barrier(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps,
                                  const hadi_barrier *barrier, double *J, double *base_prices);

/* Forward-start options and cliquets: strike fixings -- NOT a reference feature.  A cliquet sweep is the sweep of
 * hadi_DO_timestepping (variant HADI_EU or HADI_DIV) with one addition: after the last pass of every listed fixing step n, every
 * instance k that lists n takes, on every v-row j, boundary rows included,
 *     c_j     = U(i_ref, j)                      read before anything of the event is written
 *     U(i, j) <- a_i * c_j + w * P(i, j)         for every node i = 0 .. m1 (the term w * P only when w != 0)
 * The Heston problem is homogeneous in (s, K): at a fixing date the value for the as-yet-unknown strike is the value at ONE
 * reference node of each v-row, scaled along the row.
 *   i_ref     the node of the instance's own vec_s where ref_spot_i[k] sits, by the price pick's rule: the first node within 1e-10.
 *             None: HADI_ERR_NOT_ON_GRID.
 *   a_i       HADI_FIX_SHARES: a_i = s_i / s_{i_ref} (a payoff in currency whose strike is proportional to the fixing spot;
 *             a_{i_ref} is exactly 1).  HADI_FIX_RETURN: a_i = 1 (a payoff that is a function of the return S / S_fix; after the
 *             event the row is flat).
 *   w         the weight of that fixing date, weights[row][q], parallel to the schedule; NULL = all weights 0.
 *   P         the payoff field of the Bermudan calls: p->U_0, or the initial p->U where U_0 is NULL.  Read only where w != 0.
 * Step n is time to maturity n delta_t_k on the instance's own clock; n = N_k is the valuation date.  A dividend acts at the START
 * of its step, the fixing at its END; a step may carry both.  With a predictor-corrector scheme the fixing follows the corrector's
 * column pass.  Exactly: SHARES with w = 0 leaves node (i_ref, j) with its bits; RETURN with w = 0 leaves every node of row j with
 * c_j's bits; n_fix == 0 is the plain European call: same route, same bits.
 * MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's, as for barriers.
 * A forward-start call: initial condition (s - k S_ref)^+, one fixing at step (T - t1) / delta_t, SHARES, no weights, the price
 * read at S_0.  A cliquet with coupons paid at the fixing dates: initial condition f(s / S_ref) (the local-return payoff),
 * fixings at the period starts, RETURN, weights 1, put boundary data (they keep the s_max edge flat); coupons paid at maturity:
 * weights exp(-r_d n delta_t), computed by the caller.
 *   fix_steps host array [fix_rows][n_fix], the rules of ex_steps above; weights host [fix_rows][n_fix] or NULL, entries behind a
 *             zero step are ignored.
 * hadi_cliquet_timestepping reads and writes p exactly as hadi_bermudan_timestepping does (per-instance parameters, (N_i,
 * delta_t_i), put data with strike_i, dividends, scheme, memory space); the two launchers rebuild the v-grid and honour V_0_i as
 * the Bermudan launchers do, and the six groups of a Jacobian share their instance's reference spot, mode, schedule and weights.
 * The LDS-resident whole-loop kernels apply the event inside their time loop; the streaming kernels are followed by
 * hadi_fixing_gather_kernel and hadi_fixing_kernel on the steps that some instance lists.  A cliquet call never takes
 * hadi_sweep_resident or hadi_team_kernel.
 * Not covered: a reference spot between two nodes; fixings combined with exercise, knock-out or the ladder in one call; globally
 * capped cliquets (truly path-dependent).
 * Errors: HADI_AM / HADI_AM_DIV or HADI_STATE_FP32: HADI_ERR_UNSUPPORTED; a schedule that breaks the rules, a NULL struct, NULL
 * ref_spot_i with n_fix > 0, a non-finite reference spot or weight, a mode other than 0 or 1, SHARES with ref_spot <= 1e-10 (node 0
 * is the grid's 0), a NULL output: HADI_ERR_INVALID; everything the underlying entry point refuses keeps its status. */
enum hadi_fixing_mode { HADI_FIX_SHARES = 0, HADI_FIX_RETURN = 1 };
typedef struct hadi_cliquet {
    const double *ref_spot_i; /* host [n], required when n_fix > 0 */
    const int *mode_i;        /* host [n] or NULL (= SHARES) */
    int n_fix;
    const int *fix_steps;
    int fix_rows;          /* [fix_rows][n_fix], the rules of ex_steps */
    const double *weights; /* host [fix_rows][n_fix] or NULL (= 0) */
} hadi_cliquet;
int hadi_cliquet_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_cliquet *cliquet);
int hadi_compute_base_prices_cliquet(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_cliquet *cliquet,
                                     double *base_prices);
int hadi_compute_jacobian_cliquet(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps,
                                  const hadi_cliquet *cliquet, double *J, double *base_prices);

/* The Bates model: Heston plus compound-Poisson lognormal jumps in the spot -- NOT a reference feature.  In time to maturity
 *     u_t = L_Heston u + lambda (E[u(s Y)] - u - kbar s u_s),   ln Y ~ N(mu, sigma^2),   kbar = exp(mu + sigma^2 / 2) - 1.
 * A jump sweep is the sweep of hadi_DO_timestepping (variant HADI_EU or HADI_DIV, any scheme, calls and puts) with one addition:
 * after the last pass of EVERY step n <= N_k, every v-row of instance k takes  U_row <- U_row + a_k (G U_row),  a_k = lambda_k
 * delta_t_k.  G = J - I - kbar diag(s) D is the generator of the jump term on the instance's own s-grid, row 0 (s = 0) all zero:
 * J[i][l] = E[phi_l(s_i Y)] for the hat functions phi_l of the piecewise-linear interpolant (the last interval's two linear
 * pieces continued beyond s_max), D the three-point central first-derivative stencil on the non-uniform grid (the two-point
 * backward difference at i = m1).  G annihilates constants and the function s.  The splitting is first order in time.
 * MODELLING STATEMENT: the boundary data of the sweep stay the vanilla option's.  A dividend acts at the START of its step, the
 * jump sub-step at its END.
 *   lambda, mu, sigma     the jump law of every instance, unless the matching array is given
 *   lambda_i, mu_i, sigma_i   host arrays [n] or NULL
 *   shared_grid           the caller's promise that every instance has instance 0's s-grid: with (mu, sigma) shared too, ONE matrix
 *                         is built and staged for the whole batch.  The promise is checked on the device (bit-equal rows of vec_s);
 *                         a broken promise is HADI_ERR_INVALID.  0: one matrix per instance.
 * The matrices are built on the device on every call from the sweep's own s-grids (hadi_jump_matrix_kernel); the six solves of a
 * Jacobian row share their instance's matrix; hadi_compute_jacobian_bates keeps the five columns (kappa, eta, sigma, rho, V_0): the
 * jump parameters are inputs (hadi_compute_jacobian_bates_jumps below has them as columns).
 * If every a_k is 0 the call is the plain call bit for bit, on whatever route that takes; an instance
 * with a_k = 0 inside a jump call equals its plain solve bit for bit.  A jump call of this block (one without samples) runs the streaming kernels followed by
 * hadi_jump_kernel on the fp64 matrix core: never a whole-loop LDS kernel, hadi_sweep_resident or hadi_team_kernel.
 * hadi_bates_timestepping reads and writes p exactly as hadi_DO_timestepping does; the two launchers rebuild the v-grid and
 * honour V_0_i as hadi_compute_base_prices / hadi_compute_jacobian do.
 * Errors: HADI_AM / HADI_AM_DIV, HADI_STATE_FP32, a grid that takes the sequential passes (m1 > 1024 or m2 > 527):
 * HADI_ERR_UNSUPPORTED; a NULL struct, a non-finite field, lambda < 0, sigma <= 0, lambda_k delta_t_k > 1 (the weight of the
 * identity would turn negative), a broken shared_grid promise, a NULL output: HADI_ERR_INVALID; everything the underlying entry
 * point refuses keeps its status. */
typedef struct hadi_jumps {
    double lambda, mu, sigma;                /* shared */
    const double *lambda_i, *mu_i, *sigma_i; /* host [n] or NULL */
    int shared_grid;                         /* caller's promise: every instance has instance 0's s-grid */
} hadi_jumps;
int hadi_bates_timestepping(hadi_ctx *ctx, const hadi_problem *p, const hadi_jumps *jumps);
int hadi_compute_base_prices_bates(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, const hadi_jumps *jumps,
                                   double *prices);
int hadi_compute_jacobian_bates(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_jumps *jumps,
                                double *J, double *base_prices);
/* The Jacobian with the jump law among its columns: J [n][8], columns kappa, eta, sigma, rho, V_0, lambda, mu_J, sigma_J, all forward
 * differences with the one step eps; base_prices [n].  Nine groups of ONE batched sweep: the groups 0 .. 5 exactly as in
 * hadi_compute_jacobian_bates, group 6 with a_k = (lambda_k + eps) delta_t_k on the base matrix, group 7 on the matrix of (mu_k + eps,
 * sigma_k), group 8 on the matrix of (mu_k, sigma_k + eps) -- three matrix sets, each one matrix per instance, or one for the batch
 * with shared_grid and a shared (mu, sigma); per-instance lambda_i / mu_i / sigma_i are bumped per instance.  The sub-step is
 * hadi_jump_sel_kernel: hadi_jump_kernel's arithmetic, the matrix picked by group and source instance.  With per-instance matrices
 * the groups 0 .. 6 of an instance that fall into one sub-batch share a staged strip of G (hadi_set_tuning "jump_share", default 1;
 * 0: one instance per block): which instances share a block changes no result bit.
 * Variants, schemes, calls and puts, per-instance (N, delta_t) and V_0_i, memory spaces and refusals as hadi_compute_jacobian_bates,
 * plus: (lambda_k + eps) delta_t_k > 1 is HADI_ERR_INVALID.  The call always takes the jump route (group 6 jumps even where every
 * lambda_k is 0).  An instance with lambda_k = 0 has J[k][6] == J[k][7] == 0.0 exactly: its groups 7 and 8 are skipped as its
 * group 0 is. */
int hadi_compute_jacobian_bates_jumps(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps, const hadi_jumps *jumps,
                                      double *J, double *base_prices);
/* A Bates strike x maturity surface from ONE sweep: the sample calls (hadi_sample_ladder, hadi_compute_base_prices_samples,
 * hadi_compute_jacobian_samples) with the jump sub-step of hadi_bates_timestepping at the end of every step -- behind the step's last
 * column pass, in front of the snapshot.  Nothing new is defined: a sample, the row j0, the matrices, shared_grid and its check, and
 * the weights a_k = lambda_k delta_t_k are as stated above.  Jumps are multiplicative, so the problem is as homogeneous in (s, K) as
 * Heston's: G depends on the s-grid through ratios only, and scales turn one sweep into every strike (only PROPORTIONAL dividends
 * keep that).  Snapshot q equals the call with N = snap_steps[q].
 *   out   [n][n_snap][n_samp]
 *   J     [n][n_snap][n_samp][n_par], base [n][n_snap][n_samp].  n_par = 5: the six groups of hadi_compute_jacobian_bates; n_par = 8: the
 *         nine groups and three matrix sets of hadi_compute_jacobian_bates_jumps, with its bumps, its "(lambda_k + eps) delta_t_k <= 1"
 *         rule and its zero columns 6, 7 where lambda_k = 0; any other n_par is HADI_ERR_INVALID.  Every group's samples are located
 *         on the group's own rebuilt v-grid, as in hadi_compute_jacobian_samples.
 * Admitted: HADI_EU and HADI_DIV, calls with r_f = 0, puts, delta_t_i, V_0_i (the two launchers), the predictor-corrector schemes,
 * both memory spaces.  Refused, each with its parent's status: N_i, HADI_AM / HADI_AM_DIV, HADI_STATE_FP32, call data with r_f != 0,
 * grids that take the sequential passes, lambda_k delta_t_k > 1; a NULL struct or output is HADI_ERR_INVALID.
 * If every a_k is 0 the call is the plain sample call bit for bit, on whatever route that takes, with the same words from
 * hadi_describe_last_sweep; an instance with a_k = 0 inside a jump call equals its plain solve.
 * Route: the streaming kernels with hadi_jump_kernel / hadi_jump_sel_kernel and then hadi_sample_kernel behind the step, or -- Douglas
 * steps on a grid that hadi_small_kernel admits -- hadi_small_jump_kernel: the whole time loop in one launch, the sub-step on the
 * fp64 matrix core out of LDS.  hadi_set_tuning "jump_small": 1 wherever admitted, 0 never, -1 (default) by batch size.  An instance's
 * sub-step issues the same matrix instructions in the same order on either route. */
int hadi_bates_sample_ladder(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                             const int *snap_steps, const hadi_jumps *jumps, double *out);
int hadi_compute_base_prices_bates_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, const hadi_samples *samples, int n_snap,
                                           const int *snap_steps, const hadi_jumps *jumps, double *out);
int hadi_compute_jacobian_bates_samples(hadi_ctx *ctx, const hadi_problem *p, double V_0, double eps, const hadi_samples *samples,
                                        int n_snap, const int *snap_steps, const hadi_jumps *jumps, int n_par, double *J, double *base);
/* diagnostics (tests): the natural-order generator G [m1 + 1][m1 + 1] of one grid, built by the kernel the sweep uses.
 * vec_s [m1 + 1] and G_out are HOST arrays. */
int hadi_debug_jump_matrix(hadi_ctx *ctx, int m1, const double *vec_s, double mu, double sigma, double *G_out);

/* v-grid rebuilt from (V_0, V = 5.0, d = 5.0/500) exactly as every call site of the reference
 * does (jacobian_computation.cpp:253); p->vec_v / p->delta_v are ignored. */
int hadi_compute_base_prices(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                             double *base_prices);
int hadi_compute_base_prices_american(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                                      double *base_prices);
int hadi_compute_base_prices_dividends(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                                       double *base_prices);
int hadi_compute_base_prices_american_dividends(hadi_ctx *ctx, const hadi_problem *p, double S_0,
                                                double V_0, double *base_prices);

/* J: [n][5], columns kappa, eta, sigma, rho, v0; forward differences with step eps.
 * p->U is not used as input (the reference restarts every solve from U_0); p->U_0 is required. */
int hadi_compute_jacobian(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0, double eps,
                          double *J, double *base_prices);
int hadi_compute_jacobian_american(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                                   double eps, double *J, double *base_prices);
int hadi_compute_jacobian_dividends(hadi_ctx *ctx, const hadi_problem *p, double S_0, double V_0,
                                    double eps, double *J, double *base_prices);
int hadi_compute_jacobian_american_dividends(hadi_ctx *ctx, const hadi_problem *p, double S_0,
                                             double V_0, double eps, double *J, double *base_prices);

/* Levenberg-Marquardt normal equations on this rank's rows (host arrays):
 * partial[0..24] = J^T J (row-major), partial[25..29] = J^T r, partial[30] = sum r^2.
 * The 31 doubles are what gets all-reduced across GPUs. */
int hadi_lm_partials(int n, const double *J, const double *residuals, double *partial31);
/* The same reduction on the GPU (replaces KokkosBlas gemm/gemv + the residual kernel, src/jacobian_computation.cpp:117,
 * 154, heston_calibration.cpp:271-275): J [n][5], model prices [n] and market prices [n] are DEVICE arrays (what
 * hadi_compute_jacobian wrote with HADI_MEM_DEVICE); r = market - model; the 31 doubles come back to the host array
 * partial31 -- the only data that leaves the GPU per LM iteration.  Deterministic (fixed-shape tree reduction). */
int hadi_lm_partials_device(hadi_ctx *ctx, int n, const double *J, const double *model_prices,
                            const double *market_prices, double *partial31);
/* delta = (J^T J with diagonal *(1+lambda))^-1 J^T r by 5x5 partial-pivot elimination. */
int hadi_lm_solve(const double *partial31, double lambda, double *delta5);
/* The three functions above for n_par = 1 .. HADI_LM_MAX_PAR parameters (8: hadi_compute_jacobian_bates_jumps): J [n][n_par];
 * partials = [J^T J row-major n_par^2][J^T r n_par][sum r^2], n_par^2 + n_par + 1 doubles (73 at n_par = 8); delta [n_par].
 * At n_par = 5 they are the functions above, bit for bit.  n_par outside 1 .. HADI_LM_MAX_PAR: HADI_ERR_INVALID. */
#define HADI_LM_MAX_PAR 8
int hadi_lm_partials_n(int n, int n_par, const double *J, const double *residuals, double *partials);
int hadi_lm_partials_device_n(hadi_ctx *ctx, int n, int n_par, const double *J, const double *model_prices,
                              const double *market_prices, double *partials);
int hadi_lm_solve_n(int n_par, const double *partials, double lambda, double *delta);
/* Both steps on one rank: compute_parameter_update_on_device. */
int hadi_compute_parameter_update(int n, const double *J, const double *residuals, double lambda,
                                  double *delta5);


/* ---- diagnostics (tests): the two directional passes of ONE Douglas step as operators ----------------------------
 * hadi_debug_row_pass:   Y1rhs = what the row pass of step `step` hands to the A2 solve (device_solver.hpp:236-260:
 *                        explicit stage, A1 line solve, + theta dt (b2 (e_n - e_{n-1}) - A2 U)), from p->U as U_{n-1}.
 * hadi_debug_col_solve:  X = (I - theta dt A2)^{-1} p->U  (hes_a2_shuffled_kernels.hpp:243-299), European, no projection.
 * Both run the product kernels the batch shape selects; p->U is not modified; out is [n][m] in p->memspace. */
int hadi_debug_row_pass(hadi_ctx *ctx, const hadi_problem *p, int step, double *Y1rhs);
int hadi_debug_col_solve(hadi_ctx *ctx, const hadi_problem *p, double *X);
/* out[k] = the reciprocal of x[k] exactly as the line solves of the sweep form it (v_rcp_f64 + one Newton step: within
 * 10 ulp, no IEEE division); x and out are HOST arrays of n doubles.  Tests bound its error. */
int hadi_debug_rcp(hadi_ctx *ctx, int n, const double *x, double *out);

#ifdef __cplusplus
}
#endif
#endif /* HADI_H */
