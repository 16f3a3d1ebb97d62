/*
 * vilfusion.h -- C ABI of libvilfusion.so, the MI355X (gfx950) drop-in for the arithmetic
 * behind gtsam_fusion's GraphManager / IMUManager.
 *
 * The reference has no FFI layer: the only seam on its hot path is the public C++ API of
 * VILFusion::GraphManager (gtsam_fusion/include/gtsam_fusion/GraphManager.h:40-96) and
 * VILFusion::IMUManager (gtsam_fusion/include/gtsam_fusion/IMUManager.h:22-27).  Each entry
 * point below cites the reference member it replaces.  All pointers are borrowed for the
 * duration of the call; outputs are caller-allocated; no call throws; every call returns an
 * int status (0 = VF_OK, <0 = error, message via vf_last_error()).  No torch / GTSAM types.
 *
 * Layout conventions (host side of the ABI, plain AoS, float64):
 *   quaternion (w,x,y,z);  state16 = q(4) t(3) v(3) bias_acc(3) bias_gyro(3);
 *   tangent15 = dtheta(3) dp(3) dv(3) dba(3) dbg(3);  Pose3 tangent order [rot, trans].
 *   imu record (190)     = dt, delta(9), bias_hat(6), H(9x6 row-major), R(120 packed upper)
 *   between record (28)  = q_meas(4), t_meas(3), R(21 packed upper), R^T R = cov^-1
 *   prior record (31)    = mean state16, sigma(15)
 * On the device these live as AoSoA tiles of 64 factors (DESIGN.md "Data layout in HBM").
 */
#ifndef VILFUSION_H
#define VILFUSION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VF_OK 0
#define VF_ERR_INVALID (-1)       /* bad argument */
#define VF_ERR_BAD_KEY (-2)       /* unknown / out-of-window key */
#define VF_ERR_NOT_SPD (-3)       /* covariance not symmetric positive definite */
#define VF_ERR_INDETERMINATE (-4) /* normal equations not positive definite */
#define VF_ERR_DEVICE (-5)        /* HIP runtime error */
#define VF_ERR_CAPACITY (-6)      /* window / slot capacity exceeded */
#define VF_ERR_NO_DEVICE (-7)     /* no gfx950 device visible: the library never falls back to CPU */

#define VF_STATE_DIM 16
#define VF_TANGENT_DIM 15
#define VF_IMU_RECORD 190
#define VF_BTW_RECORD 28
#define VF_PRIOR_RECORD 31
#define VF_MAX_BANDWIDTH 3
#define VF_MAX_EXTRA 8            /* "far" between factors per window (vf_engine_set_extra_between) unless the handle asks for more ... */
#define VF_MAX_FAR_LIMIT 32       /* ... through max_far_factors, up to this many */

const char* vf_last_error(void);
const char* vf_version(void);
int vf_device_count(int* count);

/* ===================================================================== engine (batch)
 * B independent windows of up to `capacity` keyframes on one GPU.  This is the form the
 * hot path takes on the device; the GraphManager handle below is an engine with B = 1. */
typedef struct vf_engine vf_engine;

typedef struct {
    uint32_t struct_size;   /* sizeof(vf_engine_opts) in the header the CALLER was compiled against; vf_engine_default_opts sets
                               it.  The struct only ever grows at its end: a caller built against an older, shorter header is
                               served with the defaults for the fields it does not know; a size the library does not know
                               (larger than its own, or 0) is refused with VF_ERR_INVALID */
    int windows;            /* B */
    int capacity;           /* keyframes per window, rounded up to a multiple of 64 */
    int bandwidth;          /* max |a-b| of a between factor, 1..VF_MAX_BANDWIDTH */
    int device;             /* HIP device ordinal */
    double gravity[3];      /* n_gravity; MakeSharedU => (0,0,-9.81) (ImuManagerRos.cpp:16) */
    double lambda0, lambda_up, lambda_down, lambda_min, lambda_max; /* LM damping schedule */
    int chunks;             /* K4 form.  0 = chosen from the batch size: up to 128 windows -> partitioned
                               solve (chunks joined by 27-dof separators, about sqrt(n) of them for an
                               n-keyframe window: one-window latency); more windows -> one sweep per window
                               (throughput).  1 = always sweeps.  P >= 2 = partitioned solve with P chunks. */
    int cold_start;          /* != 0: every vf_engine_iterate linearises all factors (no warm start); default 0 */
    double accept_rel;       /* an LM trial is accepted iff  new cost < cost + accept_rel * cost.  Default 1e-9: the rounding
                                floor of the cost of a 1000-pose window (a sum of ~30 000 squared whitened residuals, the IMU
                                ones scaled by 5e4) is ~1e-10 of its value; with a strict "decreases" test (accept_rel = 0) a
                                converged window rejects about half of its Newton steps on the last bits of that sum, its
                                soft modes stop converging, and two float64 implementations end 1e-7 ... 1e-6 m apart
                                instead of 1e-9 (DESIGN.md "Accept rule at the floor").  Must be >= 0.
                                NOTE this accept test is the build's own.  Of gtsam::LevenbergMarquardtParams only lambdaInitial
                                (1e-5), lambdaFactor (10) and the termination tolerances (vf_engine_set_convergence) are
                                followed; GTSAM accepts a step on modelFidelity = actual / predicted decrease >
                                minModelFidelity (1e-3), which this library does not evaluate.  Where the optimum is does not
                                depend on either rule: tests/test_gpu_vs_qr_twin.py holds the result to an independent QR
                                optimiser that uses the gain-ratio test. */
    /* Refined solve (DESIGN.md "Refined solve"; csrc/vf_refine.hip).  The reference factorises by QR (GraphManager.cpp:38); the
     * device forms normal equations, whose condition number grows with the FOURTH power of the window length (a chain of
     * combined-IMU factors is a double integrator): ~1e11 at 1000 keyframes, beyond 1e19 at 10 000, where a float64 Cholesky
     * factor has the softest modes wrong by orders of magnitude and Gauss-Newton / LM creep instead of converging.  With
     * refinement every solve is followed by N conjugate-gradient corrections on (J^T J + lambda I) d = -J^T r with the
     * operator applied THROUGH J (accurate to cond(J), not cond(J)^2) and the Cholesky solve as preconditioner: each
     * correction costs one more solve with the same factor shape plus two passes over the Jacobians, and removes one of the
     * handful of modes the factor gets wrong.  -1 (default) = up to 12 corrections once a window is longer than
     * refine_min_keyframes, none otherwise (the headline windows are untouched); 0 = never; N = always N (at most 64).
     * Refining engines run the two-kernel form (K3 + K4).  Far factors of a refined engine are rows of the refinement's operator
     * too, and the Woodbury solve (band factor + the far factors' columns, computed once per trial) is its preconditioner. */
    int refine_iterations;
    int refine_min_keyframes;  /* default 1536: Gauss-Newton by normal equations alone contracts by 0.025 per update at 1 250 keyframes, 0.1 at
                                  1 500, 0.3 at 2 000, 0.7 at 3 000 and creeps beyond */
    double refine_rel_stop;    /* a window stops correcting once res . M^-1 res has fallen to this, squared, times its first value
                                  (default 1e-8), or stops being positive.  In auto mode (refine_iterations = -1) the tolerance EASES IN:
                                  1e-3 for a window of refine_min_keyframes, tightening log-linearly to this value at twice that length
                                  (what the normal equations get wrong grows smoothly with the window; a switch from no correction to
                                  "until 1e-8" at one length made a solve four times dearer from 1 500 to 1 600 keyframes); its remaining correction solves are skipped on the
                                  device (no host synchronisation).  How many corrections that takes grows with the window: 4 at
                                  1 600 keyframes, 5 at 2 500, 7 at 4 000, 9 at 6 000, 12 at 10 000 (tools/refine_trace_sizes.py) */
    /* Non-monotone LM ("excursions").  On a long window the Gauss-Newton step moves the far end by metres through
     * rotation-coupled dynamics; the stiff IMU residuals (sigma 2e-5 m) see the second-order part of that move, so the cost
     * RISES after the step (13 -> 1700 on the 10 000-pose window) and falls below its start only after one or two more
     * steps have corrected it (-> 10.78).  A monotone accept test rejects every such step and damped steps creep along the
     * valley (profiles/r04_config4_soft_mode.log; gtsam's own LM rule does the same).  With lm_excursion = W > 0 up to W
     * consecutive cost-raising trials are kept provisionally, each dividing lambda by lambda_down twice; a later trial whose
     * cost is below the cost the excursion started from accepts them all; if the W+1-th still is not, the starting point
     * is restored, lambda multiplied by lambda_up, and the trials count as rejected.  An excursion still open when a solve's
     * trials run out is undone.  Under this rule lambda PERSISTS from one solve to the next (the first starts from lambda0):
     * lambda0 = 1e-5 is six orders above the soft eigenvalues of a window long enough to be refined, and a solve of five
     * trials that starts there each time spends them all coming down, or repeats the same failed excursion for ever.  0 = the classical rule; -1 (default) = 3 on engines that refine (windows longer than
     * refine_min_keyframes), 0 otherwise. */
    int lm_excursion;
    /* Gauge floor of the fixed-lag marginal prior (vf_engine_marginalize / vf_engine_slide(marginalize = 1); no reference code:
     * the reference's iSAM2 graph never marginalises).  Every factor of a window is invariant under a global translation and
     * a rotation about gravity; what the window knows about those four directions is carried by the marginal prior alone --
     * the memory of the anchor prior (GraphManager.cpp:27-35), which decays with every marginalisation (measured on a
     * 200-keyframe window: 2e-3, 1e-4, 1e-5, 8e-7 after 100, 500, 1 000, 2 000 updates) until it is below the float64 rounding
     * of the 1e9-scale entries beside it: H becomes indefinite, LM trials are rejected at random (2 000+ updates), then solves
     * fail (3 500 updates of 1 000-keyframe windows; profiles/r05_soak_*).  gauge_floor is the value below which the
     * window's own softest eigenvalues (those of H along its global translation / yaw) are not allowed to fall: at every
     * marginalisation the eigenvalues of the prior's 4 x 4 gauge information below gauge_floor * n / 3 (n keyframes in the
     * window: a unit gauge vector of the window has 3 / n of its weight on the three keyframes the prior touches) are lifted
     * back to that.  Default 3e-4, two orders above the rounding of H's largest entries (2e-6): for 1 000 keyframes an
     * information of 0.1 on WHERE the window is -- a 3 m sigma; it constrains nothing the factors can see, and a prior whose
     * gauge information is still above it (the first tens of updates) is not touched, bit for bit.  0 = off. */
    double gauge_floor;
    /* Incremental updates: the banded form of what ISAM2::update does with relinearizeThreshold / relinearizeSkip 1
     * (GraphManager.cpp:37-43,126-127).  != 0: vf_engine_isam_step relinearises only the keyframes whose pending increment
     * reaches the threshold, and linearises, assembles and eliminates again only from the first keyframe that moved or whose
     * factors are new: forward elimination is causal in time, so the Cholesky panels in front of it stand; the sweep restarts
     * from a checkpoint of its trailing window (one per 8 keyframe slots, 0.77 KB per slot) and the back substitution stops
     * once three consecutive increments come out as they were.  The cost of an update then follows the number of keyframes
     * it touches, not the length of the window.  Same arithmetic in the same order as the one-wave whole-window sweep: with
     * wildfire = 0 the increments equal that sweep's to the bit.  Windows that hold far factors, and refining engines, take the
     * full update.  2 = the same kernels started at the window's first keyframe every time (what the incremental update is
     * checked against, bit for bit: tests/test_gpu_incremental.py).  Default 0.
     * MEASURED (DESIGN.md "Incremental updates"): on the synthetic Carla stream one update moves the estimate of a keyframe
     * 1 500 keyframes back by 2-3 mm -- the IMU chain is stiff (2e-5 m), the odometry factors soft (0.3 m), so every update
     * re-estimates tilt and bias for the whole history -- and with the reference's threshold of 1e-4 nine keyframes in ten are
     * relinearised at every update: the suffix IS the window, here as in iSAM2.  The mode pays when the threshold is
     * loose or the graph has stiff odometry; it is off by default. */
    /* VF_ABI_TAIL: the fields from here to the end of the struct were added after the first sized release (tests/test_abi.py
     * builds a caller against the struct without them) */
    int incremental;
    double wildfire;         /* incremental updates: an increment that changes by at most this in every component counts as unchanged
                                (ISAM2Params::wildfireThreshold, 1e-3 in GTSAM); default 0 = bitwise */
    double min_model_fidelity; /* > 0: LM trials are accepted by GTSAM's rule instead of accept_rel
                                (LevenbergMarquardtOptimizer::tryLambda, the optimiser commented out at GraphManager.cpp:128-129): a trial
                                is accepted iff modelFidelity = (cost - new cost) / (cost - cost of the linearised problem at delta)
                                exceeds this (LevenbergMarquardtParams::minModelFidelity = 1e-3).  The prediction needs the gradient
                                in memory: such engines run the assembly kernel (K3), not the assembling sweep; not for time-sharded
                                windows.  Where the optimum is does not depend on the rule; trial counts and lambda histories do.
                                Default 0 = the library's own test. */
    int max_far_factors;     /* far between factors a window may hold at once (vf_engine_set_extra_between; the far ends of its linear
                                far factor count).  0 = VF_MAX_EXTRA, at most VF_MAX_FAR_LIMIT.  While VF_MAX_EXTRA or fewer are alive the
                                small dense systems of the low-rank correction and of the joint marginalisation live in LDS; beyond
                                (engines made for more) in device memory, 0.7 MB per window -- the same arithmetic in the same
                                order, so the same bits for the same factors, a few times slower per system.  Every far factor alive costs six
                                Woodbury columns per trial (single-window engines: six windows of the column engine, 23 MB each at
                                1 200 slots).  Arrays a caller passes for a window's far list (vf_engine_get_extra_between,
                                vf_engine_get_linear_far) hold this many entries. */
} vf_engine_opts;
/* Solver-form switches: how the library maps the solve onto the part, not what it computes.  vf_engine_default_tuning sets the
 * measured optimum and vf_engine_create uses exactly that; a binding of the reference never touches this struct.  They are
 * fields, not environment variables, so that the library's behaviour never depends on the caller's environment; tests and
 * tools/ set them (vf_engine_create_tuned) to reach one form on purpose.  Grows at its end only, like vf_engine_opts. */
typedef struct {
    uint32_t struct_size;
    int sweep_two_sided_max; /* whole-window sweeps: up to this many windows, two waves per window eliminate from both ends
                                (latency); above, one wave per window (throughput).  Default 256; 0 = always one wave. */
    int hybrid_threshold;    /* with vf_engine_set_convergence on a sweep engine of > 128 windows: once at most this many
                                windows still take trials, K4 runs as the partitioned form.  Default 256; < 0 = never. */
    int use_hip_graph;       /* != 0: vf_engine_iterate replays its launch sequence from a captured hipGraph, re-captured whenever
                                the trial count, the warm-start tail or a scalar baked into the kernel arguments changes
                                (vf_engine_graph_info counts captures and replays).  Bit-identical to plain launches
                                (tests/test_gpu_hip_graph.py); measured no faster, the stream never runs empty (bench.py
                                `single_window.with_hip_graph`); default 0 */
    int solve_split_min;     /* whole-window sweeps (one wave per window): from this many windows on, the forward sweep and the
                                back substitution run as two kernels (same arithmetic, same bits): the back substitution needs
                                9 KB of LDS instead of 38 and runs several waves per SIMD.  Pays once the batch is a multiple
                                of the 1024 SIMDs of the part.  Default 2048; 0 = never. */
    int solve_assemble_min;  /* whole-window sweeps: from this many windows on, the forward sweep forms the block rows of the
                                normal equations itself, from the Jacobians K1 / K2 leave, and the assembly kernel (K3) is not
                                launched: H is neither written nor read back (vf_engine_read_normal assembles it on demand).
                                Same sums in another order: agrees with the two-kernel form to rounding, not to the bit.  Not
                                used while a window holds far between factors, on sharded engines, or by the partitioned
                                form; in the hybrid solve (termination rule on) the sweep half uses it and the assembly
                                kernel runs for the partitioned half only.  Default 768 (below ~500 windows the assembly
                                kernel's launch is shorter than what the sweep pays, and the sweep pays it for rejected
                                trials too); 0 = never. */
    int solve_assemble_waves; /* 1: the assembling sweep is one wave per window; 2 (default): two waves per window sharing its
                                LDS, one eliminating, one assembling the rows -- the same bits, 6-10 % faster; launched in
                                chunks of 1024 windows, the workgroups the part holds at once */
    int hybrid_active_list;  /* hybrid solves (termination rule on, > 128 windows): the one-wave sweeps take their windows from a compacted
                                list of those still taking trials, so that the active ones are dispatched first (default 1; 0 = window i
                                is workgroup i as before; same bits either way) */
    int far_batch_columns;   /* single-window engines (the GraphManager's) holding far factors: the 6 Woodbury columns per far factor
                                are solved as ONE batch on a second, internal engine -- a copy of the window's H per column, 6 windows
                                per far factor alive (made for 1, 2, 4, 8, 16, 32 factors as they come: 0.12 KB per keyframe slot and window,
                                0.14 GB and 2 ms for the first loop closure of a 1 200-slot handle) -- instead of one band solve after
                                the other (default 1; 0 = sequential columns as on batch engines; same bits) */
    int far_big_forms;       /* engines made with max_far_factors > VF_MAX_EXTRA: the small dense systems of the far factors in device
                                memory even while VF_MAX_EXTRA or fewer are alive (default 0 = the LDS forms then; same bits: what
                                tests/test_gpu_far_capacity.py compares) */
    int solve_backsub_form;  /* split and assembling sweeps: the back substitution kernel.  0 (default) = by batch: up to one window per
                                SIMD of the device (4 x its compute units, read when the engine is made) the form built for one wave
                                per SIMD -- the recursion software-pipelined, four panels in flight, more than 256 registers --, above
                                the form built for two waves per SIMD; 1 = always the two-per-SIMD form; 2 = always the
                                one-per-SIMD form.  Same arithmetic in the same order: same bits (tests/test_gpu_backsub_forms.py) */
} vf_engine_tuning;


/* Asynchronous staging (the GraphManager handle's engine runs this way; one-window engines that own their stream): with on != 0,
 * vf_engine_preintegrate (of keyframes beyond the window's end), vf_engine_set_between (up to 4 records),
 * vf_engine_marginalize, vf_engine_drop_oldest and vf_engine_set_range enqueue their work and return without waiting for the
 * device -- the marginalisation on a second stream, beside the staging of the keyframe that arrives (with far factors alive: on the
 * main stream, and the second one carries the Woodbury columns beside the window's own band solve) -- and what the device finds
 * wrong is reported by vf_engine_read_result instead of by the call: device_flags bit 0 = a preintegrated covariance was not
 * positive definite (VF_ERR_NOT_SPD of vf_engine_preintegrate), bit 1 = the pivot block of a marginalised keyframe was not,
 * bit 2 = the far ends' block (VF_ERR_INDETERMINATE of vf_engine_marginalize); the flags are cleared by the read.
 * vf_engine_read_result: the state of keyframe `slot` (estimate != 0: theta (+) delta of the reference-compat solve), the cost and the
 * LM counters of vf_engine_read_lm, in ONE synchronisation -- none at all when it follows a vf_engine_iterate whose adaptive trial
 * loop (one window under the termination rule) has read that very block to see the rule's flag up; any output may be null.  Works
 * on every engine. */
int vf_engine_set_async(vf_engine* e, int on);
/* asynchronous engines, after a solve: compute NOW, behind the solve, the marginal prior the next vf_engine_marginalize of this
 * window will need (its inputs -- the linearisation of the factors on the oldest keyframe at the solved states -- are final), so
 * that the call itself only puts it in place.  Used if nothing but appends happens in between; dropped otherwise.  The
 * GraphManager handle does this whenever its fixed-lag window is full.  A no-op on engines it does not apply to. */
int vf_engine_marginalize_ahead(vf_engine* e);
int vf_engine_read_result(vf_engine* e, int window, int slot, int estimate, double* state16, double* cost, int* accepted, int* rejected,
                          int* solve_failures, int* device_flags);
/* incremental engines (vf_engine_opts.incremental): updates made so far by vf_engine_isam_step, how many of them eliminated the
 * whole window (the first, and every one after an entry point the bookkeeping does not follow); for `window`, the keyframe slot
 * the last forward sweep started at and the slot the last back substitution stopped at (-1 on other engines) */
int vf_engine_incremental_info(vf_engine* e, int window, long* updates, long* whole_window_updates, int* first_eliminated,
                               int* last_substituted);
/* vf_engine_default_opts(o) fills the sizeof(vf_engine_opts) bytes of the header this translation unit was compiled against (the
 * macro below hands that size to the library); bindings that mirror the struct by hand (ctypes, cgo, JNI) call the function of the
 * same name, which fills the library's own size, or vf_engine_default_opts_sized with theirs. */
void vf_engine_default_opts(vf_engine_opts* o);
void vf_engine_default_opts_sized(vf_engine_opts* o, uint32_t struct_size);
void vf_engine_default_tuning(vf_engine_tuning* t);
void vf_engine_default_tuning_sized(vf_engine_tuning* t, uint32_t struct_size);
#ifndef VF_NO_SIZED_DEFAULTS
#define vf_engine_default_opts(o) vf_engine_default_opts_sized((o), (uint32_t)sizeof(vf_engine_opts))
#define vf_engine_default_tuning(t) vf_engine_default_tuning_sized((t), (uint32_t)sizeof(vf_engine_tuning))
#endif
int vf_engine_create(const vf_engine_opts* o, vf_engine** out);
int vf_engine_create_tuned(const vf_engine_opts* o, const vf_engine_tuning* t, vf_engine** out);   /* t = NULL: the defaults */
void vf_engine_destroy(vf_engine* e);

/* host -> device staging (each converts AoS records to the AoSoA device layout) */
int vf_engine_set_range(vf_engine* e, int window, int lo, int hi); /* active keyframes [lo,hi) */
int vf_engine_set_states(vf_engine* e, int window, int k0, int n, const double* state16);
int vf_engine_get_states(vf_engine* e, int window, int k0, int n, double* state16);
/* imu factor slot k holds the CombinedImuFactor X(k-1),V(k-1),X(k),V(k),B(k-1),B(k)
 * (IMUManager.cpp:68-73) */
int vf_engine_set_imu(vf_engine* e, int window, int k0, int n, const double* rec190);
/* BetweenFactor<Pose3>(X(a), X(b)) (GraphManager.cpp:86); stored in the slot of b; a < b,
 * b - a <= bandwidth; at most one between factor may end at a keyframe. */
int vf_engine_set_between(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b,
                          const double* rec28);
int vf_engine_clear_between(vf_engine* e, int window, int k0, int n);
/* "Far" between factors: BetweenFactor<Pose3> on ANY pair of keyframes a < b of a window -- wider than the band
 * (b - a > bandwidth), or a second factor ending at a keyframe that already has one (a loop closure).  iSAM2 takes any
 * pair of keys (GraphManager.cpp:83-88); the banded device solver keeps such factors out of H and applies them as a
 * low-rank correction: g gets their J^T r, and every LM trial solves (H_band + lambda I + U U^T) delta = -g by Woodbury
 * -- the band solver once more per column of U (6 per factor) and one small dense system per window.  A FALLBACK for
 * the rare window with such factors, several times slower than a band-only window; at most VF_MAX_EXTRA per window
 * (vf_engine_opts.max_far_factors raises that to VF_MAX_FAR_LIMIT).
 * The call REPLACES the window's list (n = 0 clears it); records as for vf_engine_set_between.
 * A far factor outlives the keyframe it is anchored on, as in the reference's unbounded graph (GraphManager.cpp:83-88).  When
 * its older keyframe a is MARGINALISED (vf_engine_marginalize / vf_engine_slide(.., 1)) the factor is marginalised with it,
 * exactly at the current linearisation: it leaves this list and joins the window's LINEAR far factor -- six whitened rows
 * per far end over the three keyframes of the marginal prior and all the far ends (marginalising a keyframe that several far
 * factors touch couples their far ends: they are one factor from then on) -- which every later marginalisation re-expresses
 * the same way, and whose far ends are folded into the marginal prior as they come within its reach (the leaving keyframe
 * + 3): the information of a loop closure outlives BOTH its ends, and a fixed-lag window follows the whole-history optimum
 * across them to 1e-7 m (tests/test_gpu_far_factors.py).  (Far ends count against VF_MAX_EXTRA; vf_engine_get_linear_far
 * lists them.)  A slide that does not marginalise re-anchors the
 * factor on keyframe a + 1 instead -- Z' = D^-1 Z with D the current estimate of T_a^-1 T_a+1, taken as exact -- and drops
 * the linear ones, as it drops the band factors of the keyframe that leaves.  Engines holding far factors start every solve
 * cold.  Not for time-sharded engines. */
int vf_engine_set_extra_between(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec28);
/* the window's (nonlinear) far factors as they stand, and how many far factors were transported (made linear by a
 * marginalisation, or re-anchored by a slide without one) / dropped by a slide that does not marginalise / absorbed into the
 * marginal prior over the life of the engine; any output pointer may be NULL */
int vf_engine_get_extra_between(vf_engine* e, int window, int* n, int32_t* a, int32_t* b, double* rec28, long* transported, long* ended,
                                long* absorbed);
/* the window's linear far factors: their number and the window-local keyframe each one ends at (far_end: max_far_factors ints -- VF_MAX_EXTRA by default -- or NULL) */
int vf_engine_get_linear_far(vf_engine* e, int window, int* n, int32_t* far_end);
/* the three priors of GraphManager.cpp:27-35 as one diagonal 15-row factor on keyframe k */
int vf_engine_set_prior(vf_engine* e, int window, int k, const double* rec31);
/* Robust loss on band between factors (no reference code of its own: GraphManager::addBetweenFactor takes any SharedNoiseModel,
 * noiseModel::Robust over a Gaussian among them; conventions of GTSAM's mEstimator classes).  With s the norm of the whitened
 * residual and k > 0 the loss's parameter:
 *   VF_LOSS_HUBER          rho(s) = s^2 / 2 up to s = k, k (s - k / 2) beyond       weight rho'/s = 1, k / s
 *   VF_LOSS_CAUCHY         rho(s) = (k^2 / 2) log(1 + s^2 / k^2)                    k^2 / (k^2 + s^2)
 *   VF_LOSS_GEMAN_MCCLURE  rho(s) = (1 / 2) k^2 s^2 / (k^2 + s^2)                   k^4 / (k^2 + s^2)^2
 * K2 writes such a factor in its square-root form, r^ = alpha r and J^ = (alpha I + gamma r r^T) J with alpha = sqrt(2 rho) / s and
 * gamma = alpha' / s: an ordinary least-squares factor whose cost 0.5 |r^|^2 IS rho(s) and whose gradient J^^T r^ is (rho'/s) J^T r,
 * the gradient GTSAM's reweighting gives.  Everything behind K2 -- the cost of an LM trial (vf_engine_read_lm reports the sum of
 * rho), the predicted decrease, every solve form, the refined solve, the marginalisation, vf_engine_factor_errors (rho(s), what
 * NonlinearFactor::error returns under noiseModel::Robust) -- sees that factor and knows nothing of losses.  The Gauss-Newton
 * matrix differs from GTSAM's (w J^T J): along r it weighs by rho'^2 / (2 rho), across r by 2 rho / s^2; the optimum is the same.
 * A Huber factor with s <= k is the Gaussian factor to the bit.  A robust factor that is marginalised enters the marginal prior at
 * the linearisation, hence the weight, it has at that moment.  The innovation gate (vf_engine_gate_tail) stays Gaussian. */
#define VF_LOSS_NONE 0
#define VF_LOSS_HUBER 1
#define VF_LOSS_CAUCHY 2
#define VF_LOSS_GEMAN_MCCLURE 3
/* the loss of the band between factors ending at slots b[0..n): an attribute of the SLOT.  A slot without a factor keeps it inertly;
 * vf_engine_set_between, vf_engine_ingest_tail and vf_engine_clear_between reset the slots they write to VF_LOSS_NONE, so the loss
 * is set AFTER the record is staged; vf_engine_compact moves it with its slot and vf_engine_grow carries it.  The first call that
 * sets a loss other than VF_LOSS_NONE makes the two per-slot arrays; an engine that never saw one launches what it always has.
 * A mutating call like vf_engine_set_between (on an asynchronous engine, n <= 4 enqueues and returns).  VF_ERR_INVALID: a loss id
 * outside 0..3, k not finite or <= 0 (ignored for VF_LOSS_NONE), a null pointer, a time-sharded engine; VF_ERR_BAD_KEY: a slot
 * outside the capacity.  Far factors take theirs with their list (vf_engine_set_extra_between_robust). */
int vf_engine_set_between_loss(vf_engine* e, int window, int n, const int32_t* b, const int32_t* loss, const double* k);
/* ... of slots k0 .. k0+n-1 (synchronises); VF_LOSS_NONE and k = 0 everywhere on an engine without the arrays.  Either output may be NULL. */
int vf_engine_get_between_loss(vf_engine* e, int window, int k0, int n, int32_t* loss, double* k);
/* Robust loss on far between factors (loop closures: the measurement most likely to be a false match, which no innovation gate
 * reaches).  vf_engine_set_extra_between with a loss per entry: the loss is an attribute of the list ENTRY, and as the list is
 * replaced as a whole the losses come with it -- vf_engine_set_extra_between IS this call with VF_LOSS_NONE everywhere, so a plain
 * re-send clears them.  k_linearize_extra writes such an entry in the square-root form above; everything that reads a far factor's
 * rows -- gradient, Woodbury columns and combine, the cost of a trial, the refined solve, the marginals, vf_engine_factor_errors
 * (rho(s)), the marginalisation -- sees that factor and knows nothing of losses.  A Huber entry with s <= k is the Gaussian factor to
 * the bit.  The loss stays on its entry through vf_engine_compact, vf_engine_grow and a re-anchoring slide; an entry whose older
 * keyframe is marginalised becomes rows of the window's LINEAR far factor (or part of the marginal prior) at the weight it has at
 * that linearisation, and leaves the list with its loss: linear far factors have none.  The first list that carries a loss other
 * than VF_LOSS_NONE makes the two per-entry arrays; an engine that never saw one allocates and launches what it always has.
 * VF_ERR_INVALID with nothing touched: a loss id outside 0..3, k not finite or <= 0 (ignored for VF_LOSS_NONE), a null pointer, a
 * time-sharded engine (and vf_engine_set_shard refuses an engine that holds far losses); otherwise the codes of
 * vf_engine_set_extra_between. */
int vf_engine_set_extra_between_robust(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec28,
                                       const int32_t* loss, const double* k);
/* ... read back: max_far_factors entries each (VF_MAX_EXTRA by default), in the order of vf_engine_get_extra_between; VF_LOSS_NONE
 * and k = 0 behind the list's end and on an engine without the arrays.  Either output may be NULL. */
int vf_engine_get_extra_between_loss(vf_engine* e, int window, int32_t* loss, double* k);
/* Absolute pose and position factors on keyframes (no reference code of its own: GraphManager::addBetweenFactor builds the sensor's
 * absolute pose and discards it; a GTSAM user adds PriorFactor<Pose3>(X(b), Z, model) or GPSFactor(X(b), z, model)).  A factor on
 * keyframe b ALONE, held in b's own between slot as a between factor from b - 1 whose first Jacobian is 36 exact zeros: J^T J gets
 * J_u^T J_u on block (b, b) and exact zeros on the blocks of b - 1, J^T r gets J_u^T r_u on b, the cost 0.5 |r_u|^2 -- a unary
 * factor's contribution, and everything behind K2 (assembly, every solve form, the LM decision, the refined and the incremental
 * solve, the marginals, vf_engine_factor_errors, the marginalisation, both gates) reads the slot as it reads any other.
 *   VF_ABSOLUTE_POSE      r = R Log(Z^-1 T_b), J_u = R J_r^-1(Log(Z^-1 T_b)): PriorFactor<Pose3>.  rec28 as for vf_engine_set_between:
 *                         Z = [q wxyz, t] in the world frame of the states, then the 21 words of the upper-triangular square-root
 *                         information R (R^T R = cov^-1), tangent order [rot, trans].
 *   VF_ABSOLUTE_POSITION  e = t_b - z in the world frame, r = R3 e, J_u = R3 [0 | R_b] (the retraction moves t by R_b dp): GPSFactor.
 *                         rec28 = [1, 0, 0, 0, z, R] with only the translation block of R's 21 words in use (R3, 3 x 3 upper
 *                         triangular, R3^T R3 = cov^-1; vf_absolute_position_record builds it).  The factor fills rows 3..5 of the
 *                         slot (r, Jb), the translation rows of a pose factor; rows 0..2 are exact zeros, and so is vf_engine_read_between_lin's
 *                         Ja of either kind.
 * The price is one factor per slot: keyframe b carries EITHER the band between factor that ends at it OR an absolute factor, and
 * b - 1 must be inside the window when the factor is linearised (the oldest keyframe of a window cannot take one).  When keyframe
 * b - 1 is marginalised the factor is absorbed into the marginal prior, at its linearisation of that moment -- one update earlier
 * than a unary factor strictly must be; a slide that drops instead of marginalising drops it there.  Lever arms and the alignment
 * of the sensor's datum with the world frame are the caller's.  vf_engine_factor_errors counts the factor in class
 * VF_FACTOR_BETWEEN (its `a` reads b - 1): a position factor's 3 rows are judged against the 6-row threshold.
 * The kind is an attribute of the SLOT, like the loss: vf_engine_set_absolute writes record, source b - 1, kind, and loss
 * VF_LOSS_NONE (vf_engine_set_between_loss AFTER it gives the factor a robust loss: (alpha I + gamma r r^T) 0 = 0, so a Huber or
 * Cauchy fix composes); vf_engine_set_between, vf_engine_ingest_tail and vf_engine_clear_between reset the slots they write to
 * VF_ABSOLUTE_NONE; vf_engine_compact moves it with its slot, vf_engine_grow carries it, a slide leaves it with its slot.  The first
 * call makes the per-slot array (and the loss arrays); an engine that never saw an absolute factor launches what it always has.
 * A mutating call like vf_engine_set_between (on an asynchronous engine, n <= 4 enqueues and returns).  Refused with nothing
 * touched: VF_ERR_INVALID for a kind other than the two, a null pointer, a time-sharded engine; VF_ERR_BAD_KEY for b - 1 < 0 or
 * b >= capacity. */
#define VF_ABSOLUTE_NONE 0
#define VF_ABSOLUTE_POSE 1
#define VF_ABSOLUTE_POSITION 2
int vf_engine_set_absolute(vf_engine* e, int window, int n, const int32_t* b, const int32_t* kind, const double* rec28);
/* ... of slots k0 .. k0+n-1 (synchronises); VF_ABSOLUTE_NONE everywhere on an engine without the array */
int vf_engine_get_absolute(vf_engine* e, int window, int k0, int n, int32_t* kind);
/* the record of a VF_ABSOLUTE_POSITION factor from the fix p and its 3 x 3 covariance (row-major; symmetrised).  Host only.
 * VF_ERR_NOT_SPD: the covariance is not symmetric positive definite; VF_ERR_INVALID: a null pointer, p not finite. */
int vf_absolute_position_record(const double p[3], const double cov9[9], double rec28[28]);

/* K0: IMU preintegration on the device.  Factor i (keyframe k0+i) integrates
 * steps[step_off[i] .. step_off[i+1]) (7 doubles each: dt, acc xyz, gyro xyz) with bias estimate
 * bias_hat6[i]; the result (mean, bias Jacobians, R = chol_upper(preintMeasCov^-1)) lands in the
 * factor's device record.  Replaces PreintegratedCombinedMeasurements::resetIntegrationAndSetBias
 * + integrateMeasurement as driven by IMUManager::getFactor (IMUManager.cpp:42-64). */
typedef struct {
    double acc_cov, gyro_cov, integration_cov;          /* ImuManagerRos.cpp:22-24,30-32 */
    double bias_acc_cov, bias_omega_cov, bias_acc_omega_int; /* ImuManagerRos.cpp:20-21,25,28-29,33 */
} vf_imu_params;
int vf_engine_preintegrate(vf_engine* e, int window, int k0, int n, const int32_t* step_off,
                           const double* steps7, const double* bias_hat6, const vf_imu_params* p);
int vf_engine_get_imu(vf_engine* e, int window, int k0, int n, double* rec190);
/* The INGEST half of a fixed-lag update, for every window at once -- what GraphManager::reserveNode (GraphManager.cpp:51-69)
 * and addBetweenFactor (:83-88) do for one vehicle per keyframe: window w's next IMU factor (hi[w]-1 -> hi[w]) is
 * preintegrated on the device from its raw samples steps7[step_off[w] .. step_off[w+1]) WITH THE WINDOW'S CURRENT BIAS
 * ESTIMATE (the bias of its last keyframe, read on the device: `getFactor(_lastPoseTime, time, _currentKey, getBias())`,
 * GraphManager.cpp:59), and the between factor that ends at the same keyframe is staged (btw_a[w] = source keyframe
 * slot, -1 = none; btw_rec28[w] its record).  One packed host->device copy from a pinned buffer, one kernel launch, no host
 * synchronisation; vf_engine_slide then appends the keyframe (its initial value predicted from this factor) and
 * vf_engine_iterate solves, the engine staying warm.  Errors found on the device (no free slot, covariance not SPD) are
 * reported by vf_engine_ingest_status, which also returns the last call's copy / kernel times from HIP events. */
int vf_engine_ingest_tail(vf_engine* e, const int32_t* step_off, const double* steps7, const vf_imu_params* p,
                          const int32_t* btw_a, const double* btw_rec28);
int vf_engine_ingest_status(vf_engine* e, float* h2d_ms, float* k0_ms);
/* IMU-rate prediction: for every window, the state its raw samples since the last keyframe hi[w]-1 lead to, and (flag) the
 * covariance the graph itself would assign to it.  Packed as vf_engine_ingest_tail (step_off: [B+1] offsets, steps7: 7 doubles per
 * step); a window may have no samples.  The samples are integrated as K0 integrates them, with the bias of that keyframe in the
 * current buffer; the state follows by the prediction vf_engine_predict makes; the bias is carried over.  One pinned copy (a buffer
 * of this call's own) and one launch on the engine's stream, no host synchronisation.
 *   VF_PROPAGATE_COVARIANCE     Sigma+ = B^-1 (A Sigma_ii A^T + P) B^-T: P the preintegrated covariance of the samples, A and B the
 *       unwhitened Jacobians of the combined-IMU factor at the predicted state (zero residual), Sigma_ii the keyframe's block left
 *       by the last vf_engine_marginals_ex -- the marginal of a keyframe attached to the window by this factor alone.  Tangent order
 *       of vf_engine_read_marginals, symmetric to the bit.  A window whose factorisation failed gets NaN (and a valid state).
 *   VF_PROPAGATE_FROM_ESTIMATE  start from the trial buffer's state of the keyframe (reference-compat engines: the estimate,
 *       as vf_engine_predict_from_estimate).
 * Without samples a window's result is the keyframe's state and Sigma_ii, bit for bit.  The call writes B x (16 + 225) doubles in a
 * buffer of its own, made by the first call, and nothing else: the engine's states, records, linearisations, LM state and what it
 * remembers of the last solve are untouched.  VF_ERR_INVALID: unknown flags; the covariance flag without marginal covariances, or
 * with ones that do not cover the last keyframe; a time-sharded engine.  VF_ERR_BAD_KEY: an empty window.  Never VF_ERR_CAPACITY. */
#define VF_PROPAGATE_COVARIANCE 1u
#define VF_PROPAGATE_FROM_ESTIMATE 2u
int vf_engine_propagate_tail(vf_engine* e, const int32_t* step_off, const double* steps7, const vf_imu_params* p, unsigned flags);
/* ... read back (synchronises); either pointer may be NULL.  VF_ERR_INVALID: no propagation since the engine was made or grown;
 * cov225 when the last propagation did not carry VF_PROPAGATE_COVARIANCE. */
int vf_engine_read_propagated(vf_engine* e, int window, double* state16, double* cov225);
/* ... and the last call's copy / kernel times from HIP events (synchronises on the kernel's event) */
int vf_engine_propagate_status(vf_engine* e, float* h2d_ms, float* kernel_ms);
/* Innovation gate: what the window as solved, and the IMU since, say about a between factor BEFORE it is added (no reference code:
 * the estimation-theoretic counterpart of the reference's degerate_odometry_filter, which drops odometry on a D-optimality
 * threshold).  For every window, with i = hi[w]-1 its last keyframe, the raw samples steps7[step_off[w] .. step_off[w+1]) that follow
 * it (packed as vf_engine_ingest_tail) and a candidate BetweenFactor<Pose3> from keyframe slot btw_a[w] to the keyframe j those
 * samples lead to (btw_rec28[w]: the record vf_engine_ingest_tail takes; btw_a[w] = -1: none):
 *   - the samples are integrated and x_j predicted exactly as vf_engine_propagate_tail does: state16 equals its state bit for bit;
 *   - the joint pose covariance of (a, j) follows from the appended keyframe's linear model d_j = G d_i + B^-1 n, n ~ N(0, P):
 *     Sigma_jj^pp from Sigma_ii and P, Cov(pose_j, pose_a) = (G_p Sigma_{i,a})[:, 0:6], Sigma_aa^pp from slot a -- the blocks the last
 *     vf_engine_marginals_ex left (VF_MARGINALS_TAIL is enough; a far downdate is honoured as it lies);
 *   - r, Ja, Jb: the factor's whitened residual and Jacobians at T_a of the current buffer and the predicted T_j;
 *     xi = Log(Z^-1 T_a^-1 T_j), the unwhitened innovation in [rot, trans] order;
 *   - S = I + Ja Sigma_aa Ja^T + Ja C^T Jb^T + Jb C Ja^T + Jb Sigma_jj Jb^T; nis = r^T S^-1 r (chi-square, 6 degrees of freedom
 *     when the measurement is consistent); nis_measurement = r^T r, twice the factor's error at the predicted state.
 * REACH: a = i or a = i-1.  An older keyframe would need the covariance of an earlier pose against a later full state, which the
 * selected inversion does not keep: such a window gets VF_GATE_OUT_OF_REACH, not an error (two solved keyframes any distance apart:
 * vf_engine_gate_closures below).
 * chi2_threshold: rejected is set when nis exceeds it and it is finite and positive (else nothing is rejected).  The 6-dof quantiles
 * a caller is likely to pass: 16.81 at 99 %, 22.46 at 99.9 %.
 * VF_GATE_FROM_ESTIMATE: as VF_PROPAGATE_FROM_ESTIMATE.
 * One pinned copy (buffers of this call's own) and one launch on the engine's stream, no host synchronisation.  The call writes one
 * record per window in a buffer made by the first call, and nothing else.  VF_ERR_INVALID: unknown flags; no valid marginal
 * covariances, or ones that do not cover the last keyframe; a time-sharded engine.  VF_ERR_BAD_KEY: an empty window. */
#define VF_GATE_FROM_ESTIMATE 2u
#define VF_GATE_OK 0            /* nis, nis_measurement, xi are valid */
#define VF_GATE_NONE 1          /* btw_a = -1: nothing to test */
#define VF_GATE_OUT_OF_REACH 2  /* a < i-1, a beyond i, a in front of the window or of the range the covariances cover */
#define VF_GATE_DEGENERATE 3    /* a = i with no samples: a factor between a keyframe and itself */
#define VF_GATE_NO_COVARIANCE 4 /* the window's factorisation failed, or S is not positive definite: nis is NaN (xi, nis_measurement valid) */
/* One window's result.  state16 is valid whatever the status; nis, nis_measurement and xi are NaN unless the status says otherwise.
 * A plain output struct: the caller fills struct_size (sizeof), the library writes no byte beyond it.  Grows at the end only. */
typedef struct {
    uint32_t struct_size;
    int32_t status;            /* VF_GATE_* */
    int32_t rejected;          /* 1: status is VF_GATE_OK and nis > chi2_threshold */
    int32_t reserved;
    double nis;
    double nis_measurement;
    double xi[6];
    double state16[16];
} vf_gate_result;
int vf_engine_gate_tail(vf_engine* e, const int32_t* step_off, const double* steps7, const vf_imu_params* p,
                        const int32_t* btw_a, const double* btw_rec28, double chi2_threshold, unsigned flags);
/* ... read back one window (synchronises).  VF_ERR_INVALID: no vf_engine_gate_tail since the engine was made, compacted or grown. */
int vf_engine_read_gate(vf_engine* e, int window, vf_gate_result* out);
/* ... every window's status and nis, B entries each, in one synchronisation; either pointer may be NULL */
int vf_engine_read_gate_all(vf_engine* e, int32_t* status, double* nis);
/* ... and the last call's copy / kernel times from HIP events (synchronises on the kernel's event) */
int vf_engine_gate_status(vf_engine* e, float* h2d_ms, float* kernel_ms);
/* Loop-closure gate: the same test for a between factor on ANY two solved keyframes of a window, before it is added (no reference
 * code; GTSAM users build it on Marginals::jointMarginalCovariance of the two keys).  n candidates, at most VF_CLOSURE_GATE_MAX on
 * one window: candidate i is a BetweenFactor<Pose3> from slot a[i] to slot b[i] of window window[i], lo <= a < b < hi, with the
 * record rec28[i] that vf_engine_set_between takes (a[i] = -1: none).
 *   - r, Ja, Jb: the factor's whitened residual and Jacobians at T_a and T_b of the current buffer; xi = Log(Z^-1 T_a^-1 T_b);
 *   - Sigma_J: the 12 x 12 joint covariance of the two poses (tangent order of vf_engine_read_marginals, a first), of
 *     Sigma = (J^T J + L)^-1 at lambda = 0 of EVERYTHING the window holds: the band, the marginal prior, the far factors alive at the
 *     weights their losses give them at this linearisation, the linear far factor -- far factors are always taken in (a loop-closure
 *     gate that ignores the closures already made has no meaning): there is no flag like VF_MARGINALS_FAR to ask for it;
 *   - S = I + [Ja Jb] Sigma_J [Ja Jb]^T, nis = r^T S^-1 r, nis_measurement = r^T r, rejected as vf_engine_gate_tail sets it.
 * Sigma_J comes from columns of the inverse, not from the selected inversion: the call makes the undamped factorisation at the
 * current states itself (the one vf_engine_marginals_ex makes) and solves the six unit columns of every distinct candidate
 * keyframe on its panels, from the window's smallest such keyframe to its end; with far factors alive the blocks take the low-rank
 * downdate of VF_MARGINALS_FAR.  No vf_engine_marginals_ex is needed before it, and the covariances that call left are neither read
 * nor written, nor is their validity changed.  A candidate's record and Sigma_J do not depend on what else the call holds.
 * Side effects, those of vf_engine_marginals_ex without its results: the current buffer's linearisation is rewritten (same bits), H,
 * g and the panels are overwritten, the engine is left cold; states, the LM state, the result block, factor errors, the propagation
 * and vf_engine_gate_tail's result are untouched.  Enqueues; scratch and result buffers of the call's own, made by the first call
 * and grown on demand (an engine that never calls it holds none).
 * Statuses (VF_GATE_*): OK; NONE (a = -1); OUT_OF_REACH (a >= b, or an end outside [lo, hi)); NO_COVARIANCE (the window's
 * factorisation or its far system failed, or S has a non-positive pivot: nis is NaN, xi and nis_measurement are valid).
 * VF_ERR_CAPACITY: more than VF_CLOSURE_GATE_MAX candidates on one window (nothing is touched: the last result stays readable);
 * VF_ERR_INVALID: a null pointer, n < 0, a time-sharded engine; VF_ERR_BAD_KEY: a window that does not exist. */
#define VF_CLOSURE_GATE_MAX 4
/* One candidate's result: nis, nis_measurement and xi are NaN unless the status says otherwise.  A plain output struct as
 * vf_gate_result: the caller fills struct_size, the library writes no byte beyond it.  Grows at the end only. */
typedef struct {
    uint32_t struct_size;
    int32_t status;            /* VF_GATE_* */
    int32_t rejected;          /* 1: status is VF_GATE_OK and nis > chi2_threshold */
    int32_t window;
    int32_t a, b;              /* as given */
    double nis;
    double nis_measurement;
    double xi[6];
} vf_closure_gate_result;
int vf_engine_gate_closures(vf_engine* e, int n, const int32_t* window, const int32_t* a, const int32_t* b, const double* rec28,
                            double chi2_threshold);
/* ... with flags.  VF_GATE_FROM_ESTIMATE: T_a and T_b, hence r, Ja, Jb and xi, are those of the trial buffer -- the ESTIMATE of a
 * reference-compat engine, whose current buffer is the linearisation point theta -- as vf_engine_gate_tail takes its newer end from
 * it; Sigma_J is of the linearisation at the current buffer either way, as every covariance of such an engine is.  flags = 0 is
 * vf_engine_gate_closures.  Unknown flags: VF_ERR_INVALID.  When no candidate of the call can be tested (every one NONE or
 * OUT_OF_REACH) nothing is factored and the engine is left as warm as it was: only the records are written. */
int vf_engine_gate_closures_ex(vf_engine* e, int n, const int32_t* window, const int32_t* a, const int32_t* b, const double* rec28,
                               double chi2_threshold, unsigned flags);
/* ... read back candidate `index` of the last call (synchronises); joint_cov144: Sigma_J row-major, or NULL (NaN unless the status is
 * VF_GATE_OK or S was not positive definite).  VF_ERR_INVALID: no vf_engine_gate_closures since the engine was made, compacted or
 * grown; VF_ERR_BAD_KEY: index at or beyond the number of candidates of that call. */
int vf_engine_read_closure_gate(vf_engine* e, int index, vf_closure_gate_result* out, double* joint_cov144);
/* ... every candidate's status and nis, n entries each, in one synchronisation; either pointer may be NULL */
int vf_engine_read_closure_gate_all(vf_engine* e, int32_t* status, double* nis);
/* ... the last call's copy / kernel times from HIP events (synchronises on the last kernel's event; the kernel time holds the
 * factorisation too), and the bytes of device memory the gate holds: its scratch and its results (0 and 0 on an engine that never
 * called it).  Any pointer may be NULL */
int vf_engine_closure_gate_status(vf_engine* e, float* h2d_ms, float* kernel_ms, uint64_t* scratch_bytes, uint64_t* result_bytes);

/* ---- hot-path stages (asynchronous on the engine's HIP stream) ---- */
/* K1+K2+priors: residual + whitened Jacobian of every factor, at the current (which=0) or
 * trial (which=1) states.  Replaces the linearisation inside ISAM2::update
 * (GraphManager.cpp:126). */
int vf_engine_linearize(vf_engine* e, int which);
/* K3: block-banded J^T J, J^T r of the current linearisation */
int vf_engine_assemble(vf_engine* e);
/* K4: (H + lambda I) delta = -g by block-banded Cholesky, one wavefront per window */
int vf_engine_solve(vf_engine* e);
/* K5: trial = current (+) delta ; then linearize(which=1) + accept/reject */
int vf_engine_retract(vf_engine* e);
int vf_engine_decide(vf_engine* e, int init);
/* `iterations` LM trials (linearize once, then {assemble, solve, retract, linearize(trial),
 * decide} per trial).  Replaces ISAM2::update + calculateEstimate (GraphManager.cpp:126-127).
 * Warm start: when nothing but vf_engine_slide has touched the engine since the previous
 * vf_engine_iterate, the opening linearisation covers only the appended keyframes' factors and
 * the priors, and the first assembly only the ends of windows whose last trial was rejected --
 * every other record, H row and g entry is still the one of the current states.  Results are
 * bit-identical to a cold start (which any other mutating call brings back). */
int vf_engine_iterate(vf_engine* e, int iterations);
/* ---- time-sharded windows (one window spread over the GPUs of a node; no reference code: the reference
 * is a single process.  SURVEY.md 8e / BASELINE.json configs[4]) ----
 * Every rank holds the whole window (states and factors replicated) in an engine created with the same
 * explicit chunk count (vf_engine_opts.chunks = P, a multiple of the world size).  Rank r owns the chunks
 * [r P / world, (r+1) P / world) and the keyframes they cover: vf_engine_linearize then writes the Jacobians
 * of the owned keyframes' factors only (plus a 5-slot halo) but the residual of EVERY factor, vf_engine_assemble
 * works on the owned rows, and one LM trial is
 *     assemble, solve_local, <all-gather sep>, solve_global, <all-reduce delta>, retract, linearize(trial), decide
 * i.e. TWO collectives, both the caller's (RCCL over xGMI via torch.distributed in
 * vil_sensor_fusion_amd/distributed.py; the library itself has no communication dependency):
 *   sep    the packed separator system, one slot of 2248 doubles per (chunk, window) = [27x28 | 27x28 | 27x27] + pad,
 *          chunk-major, so a rank's chunks are one contiguous slice: an in-place all-gather;
 *   delta  15 doubles per keyframe slot (non-owned entries zero) followed by one solve-failure flag per window: a sum.
 * The cost of a trial needs no exchange: every rank has every residual and takes the same accept / reject decision. */
typedef struct {
    int rank, world, windows, chunks;
    void* sep;              /* device, [chunks][windows][2248]: rank r writes chunks [r P/world, (r+1) P/world) */
    long sep_per_chunk;     /* doubles per chunk in sep (= windows * 2248) */
    void* delta;            /* device: increments of all keyframe slots (non-owned entries are zero after solve_global), */
    long delta_count;       /*         then one failure flag per window: capacity * windows * 15 + windows doubles */
    void* refine_delta;     /* device, shaped like delta: what vf_engine_solve_global leaves while a refinement is open (NULL when
                               vf_engine_opts.refine_iterations == 0) */
} vf_shard_info;
/* Geometry of the partitioned solve, host only (no device needed): an n-keyframe window is cut into `count`
 * chunks (<= chunks; fit != 0: also <= sqrt(n)); chunk c = `interior` keyframes from window-local
 * keyframe `first`, followed by 3 separator keyframes when has_separator.  vf_shard_range: the chunks
 * [chunk_lo, chunk_hi) and window-local keyframes [kf_lo, kf_hi) rank `rank` of `world` owns. */
int vf_chunk_geometry(int n, int chunks, int fit, int c, int* count, int* first, int* interior, int* has_separator);
int vf_shard_range(int n, int chunks, int fit, int rank, int world, int* chunk_lo, int* chunk_hi, int* kf_lo, int* kf_hi);
/* run every later stage on the caller's HIP stream (hipStream_t), e.g. the one its collectives use */
int vf_engine_set_stream(vf_engine* e, void* hip_stream);
int vf_engine_set_shard(vf_engine* e, int rank, int world);
int vf_engine_shard_info(vf_engine* e, vf_shard_info* out);
int vf_engine_solve_local(vf_engine* e);    /* chunk sweeps + spikes of the owned chunks */
int vf_engine_solve_global(vf_engine* e);   /* separator chain, back substitution of the owned chunks, zero the rest of delta */
int vf_engine_reset_lambda(vf_engine* e);   /* lambda := lambda0, as vf_engine_iterate does before its first trial */
/* The refined solve (vf_engine_opts.refine_iterations) on a time-sharded engine, staged like the solve: after the trial's two
 * collectives,  vf_engine_refine_begin ; N x { vf_engine_solve_local, <all-gather sep>, vf_engine_solve_global, <all-reduce
 * refine_delta>, vf_engine_refine_step } ; vf_engine_refine_end -- vf_engine_solve_local / _global work on the correction's
 * right-hand side while a refinement is open; N = vf_engine_refine_count (0: this engine does not refine now; the same on
 * every rank).  Unsharded engines do all of it inside vf_engine_solve. */
int vf_engine_refine_count(vf_engine* e, int* iterations);
int vf_engine_refine_begin(vf_engine* e);
int vf_engine_refine_step(vf_engine* e);
int vf_engine_refine_end(vf_engine* e);
/* corrections the last refined solve of `window` applied, and res . M^-1 res at its end relative to its first value */
int vf_engine_read_refine(vf_engine* e, int window, int* corrections, double* reduction);

/* The same from C (RCCL): the library issues the collectives itself, on the engine's stream, through the communicator the
 * caller hands in -- an ncclComm_t created by the caller (ncclCommInitRank: one rank per GPU), passed as void* so that this
 * header needs no RCCL header.  librccl is looked up with dlopen when one of these is first called: the library has no
 * link-time communication dependency.  vf_shard_iterate = vf_engine_iterate for a time-sharded engine (every rank calls it
 * with the same arguments; 2 x (1 + refinement corrections) collectives per LM trial); vf_shard_gn_step = vf_engine_isam_step.
 * vf_shard_exchange_plan (host only): what a rank sends -- its slice [sep_offset, sep_offset + sep_count) of the sep buffer
 * of sep_total doubles, all-gathered in place, and delta_count doubles all-reduced -- for callers that bring another
 * transport (vil_sensor_fusion_amd/distributed.py exchanges the same ranges through torch.distributed). */
int vf_shard_iterate(vf_engine* e, void* nccl_comm, int iterations);
int vf_shard_gn_step(vf_engine* e, void* nccl_comm, double relin_threshold);
int vf_shard_exchange_plan(int windows, int capacity, int chunks, int rank, int world, long* sep_offset, long* sep_count,
                           long* sep_total, long* delta_count);

/* Reference-compat solve: what the reference computes per GraphManager::solve (GraphManager.cpp:38-43,126-127) -- ONE
 * iSAM2-like update: keyframes whose pending increment reaches relin_threshold in any component (ISAM2Params::
 * relinearizeThreshold, 1e-4 in the reference) move their linearisation point there, every factor is linearised at the
 * linearisation points, ONE undamped Gauss-Newton system is solved for the increments of all keyframes, and the
 * estimate is theta (+) delta.  vf_engine_get_states then returns the linearisation points, vf_engine_get_estimate the
 * estimate; vf_engine_predict_from_estimate starts the IMU prediction of new keyframes from the estimate of keyframe
 * k0 - 1 (GraphManager.cpp:152-153).  Exact where iSAM2 is approximate (its partial back-substitution stops below the
 * wildfire threshold).  Not for sharded engines; fixed-lag marginalisation is not part of this mode. */
int vf_engine_isam_step(vf_engine* e, double relin_threshold);
/* the opening of such an update on its own -- relinearise, lambda := 0, linearise at theta -- for callers that stage the
 * solve themselves (time-sharded engines: vf_engine_assemble, vf_engine_solve_local, ..., vf_engine_retract follow) */
int vf_engine_gn_begin(vf_engine* e, double relin_threshold);
int vf_engine_predict_from_estimate(vf_engine* e, int window, int k0, int n);
int vf_engine_get_estimate(vf_engine* e, int window, int k0, int n, double* state16);

/* Optional LM termination (off by default: vf_engine_iterate runs exactly `iterations` trials).  With a
 * tolerance > 0, a window whose trial changes the cost by <= abs_tol, or by <= rel_tol * cost (an accepted
 * step that no longer pays, or a rejected one inside the rounding floor), is converged and takes no part in
 * the remaining trials of that solve: the rule of
 * gtsam::LevenbergMarquardtOptimizer (checkConvergence; LevenbergMarquardtParams defaults 1e-5 / 1e-5), the
 * optimiser commented out at GraphManager.cpp:128-129.  (0, 0) switches it off again. */
int vf_engine_set_convergence(vf_engine* e, double rel_tol, double abs_tol);

/* Fixed-lag marginalisation of every window's oldest keyframe (no reference code: the
 * reference's iSAM2 graph is unbounded): Schur complement of all factors touching it, at the
 * current linearisation, into a dense Gaussian prior on [next: 15 dof][next+1: pose][next+2:
 * pose].  Needs >= 4 keyframes per window and a preceding vf_engine_iterate / linearize. */
int vf_engine_marginalize(vf_engine* e);
/* lo += 1 on every window (call after vf_engine_marginalize) */
int vf_engine_drop_oldest(vf_engine* e);
/* slide every window by one keyframe: hi += 1 (new keyframe's state predicted from its IMU
 * factor, GraphManager.cpp:152-160), lo += 1.  marginalize != 0: the dropped keyframe is
 * marginalised into the dense prior above; marginalize == 0: the priors of GraphManager.cpp:27-35
 * are re-anchored on the new oldest keyframe at its current estimate (conditioning, overconfident). */
int vf_engine_slide(vf_engine* e, const double* prior_sigma15, int marginalize);
int vf_engine_read_marginal(vf_engine* e, int window, int* on, double* xbar48, double* L729, double* eta27);
int vf_engine_predict(vf_engine* e, int window, int k0, int n); /* states k0..k0+n-1 from k-1 */
/* Reclaim keyframe slots: move the live keyframes [shift, capacity) of every window down to slot 0
 * (states, factor records, linearisations, between sources, ranges, prior keys).  shift must be
 * a multiple of 64 and <= every window's lo.  Lets a fixed-lag smoother run indefinitely. */
int vf_engine_compact(vf_engine* e, int shift);
/* Grow every window to `new_capacity` keyframe slots (> the current capacity; rounded up to a multiple of 64): states
 * (both buffers), pending increments, factor records, between sources, priors / marginal priors, ranges and LM counters
 * are carried over on the device; the linearisation of the current states is recomputed, normal equations are not kept
 * (the next solve starts cold).  This is
 * what lets a GraphManager with lag = 0 keep the whole history the way the reference's unbounded iSAM2 graph does
 * (GraphManager.cpp:17-43), for as long as the 24 KB per keyframe slot fit in HBM.  Not for sharded engines.
 * Memory: the old and the new buffers are alive together until the copies are done -- a doubling peaks at 3x the old
 * footprint.  Cost: 36 pitched device-to-device copies (32 state planes + 4 arrays) whatever the number of windows. */
int vf_engine_grow(vf_engine* e, int new_capacity);
int vf_engine_sync(vf_engine* e);
/* vf_engine_opts.use_hip_graph: is replay active (0 once a capture failed or a caller's stream was handed in), how often the
 * launch sequence was captured, how many vf_engine_iterate calls were served by hipGraphLaunch */
int vf_engine_graph_info(vf_engine* e, int* enabled, int* captures, long* replays);
/* which form of K4 the next vf_engine_solve launches (it follows from the options, the batch and what the windows hold):
 * 0 one wave per window, one kernel; 1 the same as forward sweep + back substitution (solve_split_min); 2 the assembling
 * forward sweep + back substitution, no K3 (solve_assemble_min); 3 two waves per window from both ends; 4 partitioned;
 * 5 hybrid of the one-wave and the partitioned form (termination rule on) */
int vf_engine_solve_form(vf_engine* e, int* form);

/* ---- read-back (synchronises) ---- */
int vf_engine_read_imu_lin(vf_engine* e, int window, int which, int k0, int n, double* r15, double* J450);
/* (a factor with a robust loss, vf_engine_set_between_loss, reads back as K2 wrote it: r^ and J^ of its square-root form) */
int vf_engine_read_between_lin(vf_engine* e, int window, int which, int k0, int n, double* r6,
                               double* Ja36, double* Jb36);
/* ... its far twin: the linearisation of every entry of the window's far list (vf_engine_get_extra_between's order), max_far_factors
 * entries each -- r6 [X][6], Ja36 / Jb36 [X][36] -- of the current (which = 0) or the trial buffer; an empty entry, and every entry
 * of an engine that never held a far factor, reads as zeros; an entry with a loss as k_linearize_extra wrote it (r^, J^).  Any
 * output may be NULL. */
int vf_engine_read_extra_lin(vf_engine* e, int window, int which, double* r6, double* Ja36, double* Jb36);
int vf_engine_read_normal(vf_engine* e, int window, int k0, int n, double* Hband, double* g15);
int vf_engine_read_delta(vf_engine* e, int window, int k0, int n, double* delta15);
/* Cholesky panels of the last vf_engine_solve: per keyframe 43 rows x 16 doubles (15 used) =
 * rows of L in the keyframe's 15 columns for [k+1:15][k+2:pose 6][k+3:pose 6] (27 rows), the
 * forward-substituted rhs row (1), and L_kk^-T (15 rows, upper triangular). */
int vf_engine_read_panels(vf_engine* e, int window, int k0, int n, double* panels688);
/* Marginal covariances of every window's keyframes (no reference code: the counterpart of ISAM2::marginalCovariance /
 * gtsam::Marginals).  Enqueues, for every window: linearisation at the current states (what vf_engine_get_states returns: the
 * estimate of an LM engine, the linearisation points theta of a reference-compat one), assembly, a whole-window forward sweep
 * with lambda = 0 (forms 0-3 of vf_engine_solve_form; an engine whose solves are partitioned sweeps whole windows here), and
 * selected inversion of its panels (K4s, the block form of Takahashi's recursion).  The LM state is left as it was -- states,
 * increments, lambda, counters, done flags, sticky words, the cached result block -- and the engine is marked cold (the next
 * vf_engine_iterate gives the bits it would have given without the call); vf_engine_read_panels returns the undamped panels
 * afterwards.  Refused with VF_ERR_INVALID: time-sharded engines, and engines with far factors alive in any window, linear ones
 * included (vf_engine_get_extra_between, vf_engine_get_linear_far) -- vf_engine_marginals_ex with VF_MARGINALS_FAR takes those.
 * The blocks live in a device array of 2.7 KB per keyframe slot, allocated by the first call.  = vf_engine_marginals_ex(e, 0). */
int vf_engine_marginals(vf_engine* e);
/* vf_engine_marginals with flags.  VF_MARGINALS_FAR: far factors alive (linear ones included) are no longer refused; their
 * Jacobians at the current states correct the band's covariances by a low-rank downdate, Sigma = A^-1 - Z C^-1 Z^T with A the
 * undamped band, U the whitened far rows (m = 6 x slots in use), Z = A^-1 U and C = I + U^T Z, solved on the panels of the one
 * factorisation the call makes (the factorisation vf_engine_marginals makes on the same engine without far factors).  Same
 * output, same read-back; windows without a live far factor get exactly the bits vf_engine_marginals gives them on that engine,
 * and an engine without far factors gives them everywhere.  A window whose C is not positive definite reads back VF_ERR_NOT_SPD.
 * The LM state is untouched as above, and so are the far lists, the linear far factor, the marginal prior computed ahead
 * (vf_engine_marginalize_ahead) and the column engine.  The call's scratch (M x 15 x m + m^2 doubles per window) is allocated by
 * the first such call and kept; it is bounded by 1 GiB: more windows than fit are done in groups.  Unknown
 * flags: VF_ERR_INVALID. */
#define VF_MARGINALS_FAR 1u
/* VF_MARGINALS_POSE (may be combined with VF_MARGINALS_FAR): behind the selected inversion, and the far downdate where there is
 * one, the same call leaves three more device arrays for every keyframe of every window's range -- what the degeneracy metrics
 * take (vf_engine_marginal_scores), allocated by the first call that carries the flag (624 B per keyframe slot):
 *   cov36   the pose covariance in nav_msgs/Odometry order (x, y, z, rx, ry, rz), row-major: A Sigma_pp A^T with Sigma_pp the
 *           leading 6 x 6 of the keyframe's block, A = diag(R, R) P, P the swap [omega, v] -> [v, omega] and R the rotation of the
 *           state this very call linearised at (the states may move on afterwards while the covariances stay readable);
 *   info36  its inverse, by a 6 x 6 Cholesky factorisation (NaN throughout where a pivot is not positive);
 *   pose6   (x, y, z, roll, pitch, yaw) of that state, angles in the static x-y-z convention of tf.transformations.euler_from_quaternion.
 * cov36 and info36 are symmetric to the bit.  A window whose factorisation failed holds NaN in all three.  Without the flag the
 * call launches what it always launched, gives the same bits and allocates nothing more. */
#define VF_MARGINALS_POSE 2u
/* VF_MARGINALS_TAIL: the blocks of every window's last two keyframes only (slots hi-1 and hi-2: what vf_engine_gate_tail and
 * vf_engine_propagate_tail read).  The selected inversion walks backward from hi-1 and stops after two steps instead of hi-lo; the
 * factorisation in front of it is the same, and the blocks written are bit for bit those of the full call.  The range the
 * covariances cover becomes [max(lo, hi-2), hi): reads below it are refused with VF_ERR_BAD_KEY as any read outside the range is.
 * Combined with VF_MARGINALS_FAR or VF_MARGINALS_POSE: VF_ERR_INVALID. */
#define VF_MARGINALS_TAIL 4u
int vf_engine_marginals_ex(vf_engine* e, unsigned flags);
/* ... read back (synchronises): for keyframes k0 .. k0+n-1 of the range the last vf_engine_marginals saw, Sigma_kk (full
 * symmetric 15x15, row-major) and the cross block Sigma_{k+1,k} (15x15, row = dof of k+1, column = dof of k; zero for the window's
 * last keyframe).  Tangent order [omega, v] of Pose3, velocity, bias [acc, gyro].  Either pointer may be NULL.  VF_ERR_NOT_SPD:
 * the window's undamped normal equations are not positive definite; VF_ERR_INVALID: no vf_engine_marginals since the engine was
 * made, compacted or grown; VF_ERR_BAD_KEY: outside that range. */
int vf_engine_read_marginals(vf_engine* e, int window, int k0, int n, double* cov225, double* cross225);
/* ... and the records of VF_MARGINALS_POSE (synchronises): n x 36, n x 36 and n x 6 doubles; any pointer may be NULL.  Refusals as
 * vf_engine_read_marginals; VF_ERR_INVALID also when the last vf_engine_marginals_ex did not carry VF_MARGINALS_POSE. */
int vf_engine_read_pose_marginals(vf_engine* e, int window, int k0, int n, double* cov36, double* info36, double* pose6);
/* Degeneracy scores of those records, on the device (K6 over windows; the reference's online node per message:
 * vil_fusion/src/vil_fusion/degeneracy_detection.py:82-130).  Enqueues one launch over every window: `metric` (VF_METRIC_*) on the
 * subsets of subset_mask (as vf_degeneracy_scores_batch), of the pose covariances (VF_SCORE_COVARIANCE) or their inverses
 * (VF_SCORE_INFORMATION).  Each window's range is a time series of its own: the score of its first keyframe is 0 and no keyframe is
 * compared with one of another window.  The values are bit for bit what vf_degeneracy_scores_batch returns for the window's
 * records (vf_engine_read_pose_marginals) alone; kullback_leibler takes its poses from pose6.  The scores live in a device array
 * sized for the rows asked for and grown on demand.  VF_ERR_INVALID: unknown source, metric or mask; no pose marginals (none
 * computed, or the engine was compacted or grown since). */
#define VF_SCORE_COVARIANCE 0
#define VF_SCORE_INFORMATION 1
int vf_engine_marginal_scores(vf_engine* e, int source, int metric, unsigned subset_mask);
/* ... read back (synchronises): popcount(subset_mask) rows of n values, in ascending subset id, of the last
 * vf_engine_marginal_scores (its metric and mask), for keyframes k0 .. k0+n-1.  VF_ERR_INVALID: no scores since the last
 * vf_engine_marginals_ex; VF_ERR_BAD_KEY: outside the range the marginals were computed for; VF_ERR_NOT_SPD: a failed window. */
int vf_engine_read_marginal_scores(vf_engine* e, int window, int k0, int n, double* out);
/* Per-factor chi-square errors and a consistency summary (no reference code: the counterpart of NonlinearFactor::error,
 * NonlinearFactorGraph::error and printErrors, which the reference never calls).  The error of a factor is e = 0.5 |r|^2 of its
 * whitened residual r at the window's current states (what vf_engine_get_states returns: the estimate of an LM engine, the
 * linearisation points theta of a reference-compat one); the errors of a window add up to the cost vf_engine_read_lm reports.
 * Enqueues one launch over every window (kernels/kerr.inc) and one over their summaries.
 *   flags = 0: the residuals the last solve left in the current buffer are read as they lie, provided the engine can vouch that
 *     they are of the current states -- nothing has been written since a vf_engine_iterate, vf_engine_isam_step,
 *     vf_engine_linearize(e, 0) or vf_engine_marginals_ex ended, other than records at or beyond the end of a one-window engine's
 *     window.  Such a call touches nothing but its own buffer: warm start, the marginal prior computed ahead, the cached result
 *     block, covariances and scores are as they were.
 *   VF_ERRORS_RELINEARIZE, or an engine that cannot vouch (always: engines with lm_excursion active or incremental != 0): every
 *     factor is first linearised at the current states, as vf_engine_marginals does -- the same bits into the same buffer, LM state
 *     untouched, engine marked cold (the next vf_engine_iterate gives the bits it would have given without the call).
 * chi2_threshold6 (may be NULL: nothing is flagged): per class, a factor counts as flagged when 2 e exceeds the class's threshold; an
 * entry that is not a finite positive number flags nothing in its class.
 * The results live in a device buffer of their own (16 B per keyframe slot, 2 x max_far_factors doubles and one summary per window),
 * made by the first call.  They are of the call that wrote them: later solves leave them readable, the next call replaces them,
 * vf_engine_compact and vf_engine_grow void them.  VF_ERR_INVALID: unknown flags, time-sharded engines. */
#define VF_ERRORS_RELINEARIZE 1u
#define VF_FACTOR_IMU 0
#define VF_FACTOR_BETWEEN 1
#define VF_FACTOR_PRIOR 2
#define VF_FACTOR_MARGINAL_PRIOR 3
#define VF_FACTOR_FAR 4
#define VF_FACTOR_FAR_LINEAR 5
#define VF_FACTOR_CLASSES 6
#define VF_CONSISTENCY_NONFINITE 1u /* vf_consistency.status: some factor's error is not finite */
#define VF_CONSISTENCY_FLAGGED 2u   /* ... some factor is flagged */
#define VF_CONSISTENCY_EMPTY 4u     /* ... the window holds no keyframe */
/* One window's summary, per class VF_FACTOR_*: the number of factors, the sum of their errors, the largest and where it sits (a
 * keyframe slot for classes 0 .. 3 -- the slot a band factor ends at, the prior's slot, the window's first slot for the marginal
 * prior --, an index of vf_engine_read_far_errors for classes 4 and 5; the lowest of a tie; max = -1 and argmax = -1 when there is
 * none), how many are flagged, how many are not finite.  Errors that are not finite are counted in nonfinite and enter neither
 * sum nor max.  total: the six sums added in class order.  rows: whitened rows, 15, 6, 15, 27, 6 and 6 per factor by class;
 * unknowns = 15 x keyframes.  A plain output struct: the caller fills struct_size (sizeof), the library writes no byte beyond it;
 * 0 or a size larger than the library's is VF_ERR_INVALID.  Grows at the end only. */
typedef struct {
    uint32_t struct_size;
    uint32_t status;           /* VF_CONSISTENCY_* bits */
    int32_t count[6];
    int32_t argmax[6];
    int32_t flagged[6];
    int32_t nonfinite[6];
    double sum[6];
    double max[6];
    double total;
    int32_t keyframes;
    int32_t rows;
    int32_t unknowns;
    int32_t reserved;
} vf_consistency;
/* The whole batch, from the summaries and the LM words at the time of the call (the lifetime counters of vf_engine_read_lm): windows
 * that are empty; with n_fail > 0; whose cost or any factor's error is not finite; non-empty ones that never accepted a trial; with
 * a flagged factor; and the window with the largest reduced chi-square 2 total / max(rows - unknowns, 1) (the lowest of a tie; -1
 * and 0.0 if every window is empty).  struct_size as in vf_consistency. */
typedef struct {
    uint32_t struct_size;
    int32_t windows;
    int32_t empty;
    int32_t failed;
    int32_t nonfinite;
    int32_t never_accepted;
    int32_t flagged_windows;
    int32_t worst_window;
    double worst_reduced_chi2;
} vf_batch_health;
int vf_engine_factor_errors(vf_engine* e, unsigned flags, const double* chi2_threshold6);
/* ... read back (synchronises): for keyframe slots k0 .. k0+n-1 of the range the call saw, the error of the IMU factor and of the
 * band between factor ending at each slot (-1: none -- the window's first slot has no IMU factor) and the slot that between factor
 * starts from (-1: none).  Any pointer may be NULL.  VF_ERR_INVALID: no vf_engine_factor_errors since the engine was made, compacted
 * or grown; VF_ERR_BAD_KEY: outside that range. */
int vf_engine_read_factor_errors(vf_engine* e, int window, int k0, int n, double* imu_err, double* btw_err, int32_t* btw_a);
/* ... the far factors' errors, max_far_factors entries each (vf_engine_opts; 8 by default): far_err[i] of entry i of the window's
 * list (vf_engine_get_extra_between), far_linear_err[s] of far end s of its linear far factor (vf_engine_get_linear_far); -1: none */
int vf_engine_read_far_errors(vf_engine* e, int window, double* far_err, double* far_linear_err);
int vf_engine_read_consistency(vf_engine* e, int window, vf_consistency* out);
int vf_engine_read_health(vf_engine* e, vf_batch_health* out);
int vf_engine_read_lm(vf_engine* e, int window, double* cost, double* lambda, int* accepted,
                      int* rejected, int* solve_failures);
/* non-monotone LM: trials kept provisionally so far (not counted in accepted / rejected), and whether an excursion is open */
int vf_engine_read_excursions(vf_engine* e, int window, int* provisional_trials, int* open_now);
/* non-monotone LM: undo an excursion that is still open (restore the point it started from).  vf_engine_iterate does this
 * after its last trial; callers that stage their trials (time-sharded windows) call it after theirs. */
int vf_engine_close_excursions(vf_engine* e);

/* ---- measurement: time `reps` launches of one stage with HIP events on the engine stream ---- */
#define VF_STAGE_LINEARIZE_IMU 1
#define VF_STAGE_LINEARIZE_BTW 2
#define VF_STAGE_ASSEMBLE 3
#define VF_STAGE_SOLVE 4
#define VF_STAGE_RETRACT 5
#define VF_STAGE_DECIDE 6
#define VF_STAGE_ASSEMBLE_IDLE 7   /* K3 when every window's last trial was rejected: nothing to assemble, the cost of its launch */
int vf_engine_time_stage(vf_engine* e, int stage, int reps, float* avg_ms);
/* HIP-event time of a whole vf_engine_iterate(iterations) */
int vf_engine_time_iterate(vf_engine* e, int iterations, float* ms);
int vf_engine_counts(vf_engine* e, int64_t* n_imu, int64_t* n_between, int64_t* n_keyframes);

/* ===================================================================== degeneracy metrics (K6)
 * Batched form of the reference's per-message metric calls:
 *   y[0] = 0 ; y[i] = metric(mat_now = mats[i], mat_prev = mats[i-1], pose_now, pose_prev)
 * (apply_degen_function, vil_fusion/python/make_prettier_graphs.py:547-576).
 * mats: (count,6,6) row-major; pose: (count,6) [x y z roll pitch yaw] or NULL; dtype 0 = f64,
 * 1 = f32 (mats/pose/out all of that type); subset 0 = all 6x6, 1 = trans [0:3,0:3],
 * 2 = rot [3:6,3:6], 3 .. 8 = the 1x1 diagonal entry (and pose component) of x, y, z, roll, pitch,
 * yaw (make_prettier_graphs.py:555-558).  metric ids follow degen_funcs
 * (vil_fusion/python/degeneracy_detection_functions.py:283-303) then condition_number,
 * differential_entropy, then the variants jensen_bregman_0, kullback_leibler_0pose,
 * kullback_leibler_0cov (:184-193) and condition_cov (:247-251).  kullback_leibler needs pose;
 * kullback_leibler_0pose ignores it (pose may be NULL).  kullback_leibler_0cov inverts the zero
 * matrix in the reference, which raises and is caught: it is NaN for every message (y[0] = 0) and
 * computes nothing.  condition_cov is the exact negation of condition_number.
 * reps/kernel_ms: optional HIP-event timing of the kernel alone. */
#define VF_METRIC_D_OPT 0
#define VF_METRIC_D_OPT_RATIO 1
#define VF_METRIC_A_OPT 2
#define VF_METRIC_A_OPT_RATIO 3
#define VF_METRIC_E_OPT 4
#define VF_METRIC_E_OPT_RATIO 5
#define VF_METRIC_MAX_EIGEN 6
#define VF_METRIC_MAX_EIGEN_RATIO 7
#define VF_METRIC_JENSEN_BREGMAN 8
#define VF_METRIC_CORRELATION_MATRIX_DISTANCE 9
#define VF_METRIC_KULLBACK_LEIBLER 10
#define VF_METRIC_NORM_FROBENIUS 11
#define VF_METRIC_NORM_FROBENIUS_RATIO 12
#define VF_METRIC_NORM_NUCLEAR 13
#define VF_METRIC_NORM_NUCLEAR_RATIO 14
#define VF_METRIC_NORM_1 15
#define VF_METRIC_NORM_1_RATIO 16
#define VF_METRIC_NORM_2 17
#define VF_METRIC_NORM_2_RATIO 18
#define VF_METRIC_CONDITION_NUMBER 19
#define VF_METRIC_DIFFERENTIAL_ENTROPY 20
#define VF_METRIC_JENSEN_BREGMAN_0 21
#define VF_METRIC_KULLBACK_LEIBLER_0POSE 22
#define VF_METRIC_KULLBACK_LEIBLER_0COV 23
#define VF_METRIC_CONDITION_COV 24
#define VF_SUBSET_ALL 0
#define VF_SUBSET_TRANS 1
#define VF_SUBSET_ROT 2
#define VF_SUBSET_X 3
#define VF_SUBSET_Y 4
#define VF_SUBSET_Z 5
#define VF_SUBSET_ROLL 6
#define VF_SUBSET_PITCH 7
#define VF_SUBSET_YAW 8
int vf_degeneracy_batch(const void* mats, const void* pose, int count, int dtype, int subset, int metric,
                        void* out, int reps, float* kernel_ms);
/* extra: the three metrics that read the ends of the spectrum -- e_opt, max_eigen, condition_number
 * (degeneracy_detection_functions.py:74-82, 98-106, 239-243) -- of ONE eigen-solve per matrix, one launch, three outputs (each `count`
 * values, [0] = 0): bit for bit what three vf_degeneracy_batch calls return, at a third of the work.  condition_number is NaN for a
 * matrix that is not symmetric to rounding (its singular values are then not the moduli of its eigenvalues: ask
 * vf_degeneracy_batch, which falls back to an SVD).  Subsets 3 .. 8 (1x1): e_opt = max_eigen = the entry,
 * condition_number = -1 (-inf for a zero entry). */
int vf_degeneracy_spectrum_batch(const void* mats, int count, int dtype, int subset, void* e_opt, void* max_eigen,
                                 void* condition_number, int reps, float* kernel_ms);
/* Several subsets of one metric in one launch (the online node's score_all / score_trans / score_rot,
 * vil_fusion/src/vil_fusion/degeneracy_detection.py:115-130): every matrix is read from memory once.
 * subset_mask: bit s = subset s (VF_SUBSET_*), bits 0 .. 8 only, at least one.  out holds
 * popcount(subset_mask) rows of `count` values, in ascending subset id, each row bit for bit what
 * vf_degeneracy_batch returns for that subset (row[0] = 0).  Other arguments as vf_degeneracy_batch. */
int vf_degeneracy_scores_batch(const void* mats, const void* pose, int count, int dtype, int metric, unsigned subset_mask,
                               void* out, int reps, float* kernel_ms);
/* The shipped gate (gtsam_fusion/src/degerate_odometry_filter.cpp:29-47): float32 log det of the
 * rotation (3,3) and translation (0,0) 3x3 blocks of the 36-float LOAM Hessian; keep[i] = 0 when
 * either is below its threshold (fusion_params.yaml:35-36: 11.5 / 28.9). */
int vf_dopt_filter_f32(const float* hessians36, int count, float rot_thr, float trans_thr, float* rot_dopt,
                       float* trans_dopt, unsigned char* keep);
/* Deweight instead of drop: the covariance of an odometry increment from the scan-matching Hessian of its scan, which keeps
 * what the scan observed and lets go of what it did not (no reference code: the shipped gate above drops the message).
 *   Hs = (H + H^T) / 2;  H' = D Hs D, D = diag(trans_thr^-1/2 x 3, rot_thr^-1/2 x 3);  H' = V diag(l') V^T;
 *   g_i = clamp(l'_i, floor, 1);  Sigma = N + N^1/2 [sum_i (1 / g_i - 1) v_i v_i^T] N^1/2,  N = diag(nom6);
 *   R = chol_upper(Sigma^-1), Sigma^-1 = N^-1/2 V diag(g) V^T N^-1/2 formed without an inversion.
 * hessians36: (count,6,6) row-major in LOAM / ROS order [trans 3, rot 3], dtype 0 = f64, 1 = f32 (promoted on load: all
 * arithmetic and every output is float64, and a float32 call returns the bits of the float64 call on the promoted values).
 * nom6: the nominal covariance of each axis in the same order, > 0; trans_thr, rot_thr > 0: the eigenvalue at and above
 * which a direction counts as observed (exp(28.9 / 3) and exp(11.5 / 3) give a 3x3 block with every eigenvalue at the
 * threshold the log det the shipped gate tests); floor in (0, 1]: the least share of the nominal information a direction keeps.
 * out_order 0: outputs in the input order; 1: in the Pose3 tangent order [rot, trans] of vf_add_between (Sigma is permuted
 * before R is taken).  The Hessian is read in the frame of the increment's tangent; no frame change is made.
 * cov36: (count,36) row-major, symmetric to the bit; sqrt_info21 (may be NULL): (count,21), the upper triangle of R by rows --
 * words 7 .. 27 of a between record; eig6 (may be NULL): (count,6) eigenvalues of Hs (not H'), ascending; deweighted: (count)
 * the number of g_i < 1.  Where it is 0, Sigma is N and R is diag(1 / sqrt(nom6)), bit for bit.  A message with a non-finite
 * entry gets deweighted = -1, Sigma = N / floor, the matching R, and NaN in eig6.  count = 0 returns VF_OK without a device. */
int vf_degeneracy_remap_batch(const void* hessians36, int count, int dtype, const double nom6[6], double trans_thr,
                              double rot_thr, double floor, int out_order, double* cov36, double* sqrt_info21,
                              double* eig6, int32_t* deweighted, int reps, float* kernel_ms);

/* ===================================================================== GraphManager surface
 * Drop-in for VILFusion::GraphManager + VILFusion::IMUManager.  ROS-free, usable in simulated
 * time, every call thread-safe (GraphManager.h:4-6): the same two-lock discipline as the
 * reference (_graphMutex for ingestion, _stateMutex for the estimate; GraphManager.h:103-104),
 * vf_solve releases the ingestion lock before optimising and runs callbacks on the solving
 * thread inside the state lock (GraphManager.cpp:104-138). */
typedef struct vf_graph vf_graph;

typedef struct {
    uint32_t struct_size; /* sizeof(vf_graph_opts) in the caller's header (vf_graph_default_opts sets it); same rule as vf_engine_opts */
    int capacity;    /* keyframe slots on the device (keys 0..capacity-1), rounded up to a multiple of 64 by vf_create (the
                        engine allocates whole tiles); with lag = 0 the INITIAL number: vf_solve doubles it whenever the
                        history outgrows it (vf_engine_grow), unless fixed_capacity != 0 */
    int lag;         /* fixed-lag window length in keyframes; 0 = smooth the whole history */
    int iterations;  /* LM trials per vf_solve, at most (see rel_tol / abs_tol) */
    int device;
    double prior_sigma[15]; /* X0/V0/B0 prior sigmas; default GraphManager.cpp:27-31 */
    /* LM termination inside a vf_solve (vf_engine_set_convergence): the solve stops taking trials once one changes the
     * cost by <= abs_tol or <= rel_tol * cost.  Defaults 1e-5 / 1e-5 = gtsam::LevenbergMarquardtParams (the optimiser at
     * GraphManager.cpp:128-129); 0 / 0 = always `iterations` trials. */
    double rel_tol, abs_tol;
    int cold_start;  /* != 0: the handle's engine never warm-starts a solve (vf_engine_opts.cold_start); default 0 */
    int fixed_capacity; /* != 0 with lag = 0: vf_reserve_node fails with VF_ERR_CAPACITY once `capacity` keyframes exist
                           (the behaviour before the history could grow); default 0 */
    /* reference_compat != 0: vf_solve does what the reference's solve() does -- one iSAM2-like update
     * (vf_engine_isam_step with relin_threshold, default 1e-4 = GraphManager.cpp:40) instead of LM to convergence; needs
     * lag == 0 (the reference's graph is unbounded).  Default 0. */
    int reference_compat;
    double relin_threshold;
    /* incremental != 0 (with reference_compat): the update is done incrementally (vf_engine_opts.incremental -- read its
     * MEASURED note -- and .wildfire): a vf_solve costs what the keyframes it touches cost.  Default 0. */
    /* VF_ABI_TAIL: as in vf_engine_opts */
    int incremental;
    double wildfire;
    double min_model_fidelity; /* vf_engine_opts.min_model_fidelity (GTSAM's LM accept rule; 1e-3 there); default 0 = the library's own */
    int synchronous_staging;   /* != 0: the handle's engine stages synchronously, as before round 6 (every staging call waits for the
                                  device and reports its own failures; no preintegration at vf_reserve_node, no marginal prior computed
                                  ahead): same bits as the default, slower; what tests compare the asynchronous path with.  Default 0 */
    int max_far_factors;       /* vf_engine_opts.max_far_factors: loop closures (between factors the band cannot hold) alive at once;
                                  vf_add_between returns VF_ERR_CAPACITY beyond.  0 = the default, VF_MAX_FAR_LIMIT (a handle has no
                                  caller-sized arrays to keep small; while VF_MAX_EXTRA or fewer are alive it solves with the LDS forms) */
    int far_covariance;        /* != 0: vf_get_marginal_covariance and the covariance callbacks take far factors alive (loop closures, linear
                                  ones included) into account -- vf_engine_marginals_ex(VF_MARGINALS_FAR) -- instead of refusing while any is
                                  alive.  Default 0 */
} vf_graph_opts;

/* (time, pose q_wxyz, position, velocity, bias[acc,gyro]) -- GraphManager::OptimizationCallback
 * (GraphManager.h:38) */
typedef void (*vf_callback)(void* user, double time, const double q[4], const double t[3],
                            const double v[3], const double bias[6]);

void vf_graph_default_opts(vf_graph_opts* o);
void vf_graph_default_opts_sized(vf_graph_opts* o, uint32_t struct_size);
#ifndef VF_NO_SIZED_DEFAULTS
#define vf_graph_default_opts(o) vf_graph_default_opts_sized((o), (uint32_t)sizeof(vf_graph_opts))
#endif
/* GraphManager::GraphManager(imuManager) + IMUManager::IMUManager(params) + getImuParams
 * (GraphManager.cpp:15-44, IMUManager.cpp:13-17, ImuManagerRos.cpp:14-36) */
int vf_create(const vf_imu_params* imu, const vf_graph_opts* opts, vf_graph** out);
void vf_destroy(vf_graph* g);
/* extra (no reference twin): the reference anchors X(0) = identity, V(0) = 0, B(0) = 0 with the priors of
 * GraphManager.cpp:20-35, which suits a vehicle that starts level and at rest; to replay a log that starts in motion, put the
 * anchor (state16: q t v bias) and the means of the three priors somewhere else.  Only before the first vf_reserve_node. */
int vf_set_initial_state(vf_graph* g, const double state16[16]);
/* IMUManager::addIMUMeasurement (IMUManager.cpp:19-25) */
int vf_add_imu(vf_graph* g, double time, const double acc[3], const double gyro[3]);
/* GraphManager::reserveNode (GraphManager.cpp:51-69): 1-based key, key 0 is the prior node */
int vf_reserve_node(vf_graph* g, double time, uint64_t* key_out);
/* GraphManager::addBetweenFactor (GraphManager.cpp:83-88) with noiseModel::Gaussian::Covariance
 * (SensorManagerRos.cpp:99); cov is 6x6 row-major in Pose3 tangent order [rot, trans].  Any pair of reserved keys prev < cur: a
 * factor the band cannot hold (wider than VF_MAX_BANDWIDTH keyframes, or a second one ending at cur: a loop closure) is a far
 * factor (vf_engine_set_extra_between), of which vf_graph_opts.max_far_factors may be alive at once -- VF_ERR_CAPACITY beyond. */
int vf_add_between(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q_wxyz[4],
                   const double t[3], const double cov36[36]);
/* GraphManager::addBetweenFactor with noiseModel::Robust over that Gaussian: loss = VF_LOSS_* with its parameter k ("Robust loss on
 * band between factors" above; vf_engine_set_between_loss behind the record at the solve, on the synchronous and the asynchronous
 * staging path alike).  Validates as vf_add_between does, with the same codes, and VF_ERR_INVALID for an unknown loss or a k that is
 * not finite and > 0; loss = VF_LOSS_NONE is vf_add_between.  By default band factors only: a pair the band cannot hold (wider than
 * VF_MAX_BANDWIDTH keyframes, or a second factor ending at cur_key) would be a far factor -- refused with VF_ERR_INVALID, nothing
 * staged.  After vf_set_robust_far(g, 1) such a pair is staged as a far factor that carries its loss ("Robust loss on far between
 * factors" above), through every solve, marginalisation of another closure's anchor and late arrival.  Late factors that a solve
 * gives back keep their loss. */
int vf_add_between_robust(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q_wxyz[4], const double t[3],
                          const double cov36[36], int loss, double k);
/* on != 0: vf_add_between_robust accepts a pair the band cannot hold (a loop closure) and stages it as a far factor that carries its
 * loss (vf_engine_set_extra_between_robust) instead of refusing it; 0, what a new handle does: refuse.  Any time; it decides about
 * the factors added after it, the ones staged already keep what they have.  (A call, not a field of vf_graph_opts: the struct is
 * as every caller built against it knows it.)  VF_ERR_INVALID: null handle. */
int vf_set_robust_far(vf_graph* g, int on);
/* Absolute factors on the handle ("Absolute pose and position factors on keyframes" above): what a GTSAM user adds through the graph
 * as PriorFactor<Pose3>(X(key), Z, Gaussian::Covariance(cov36)) / GPSFactor(X(key), p, Gaussian::Covariance(cov9)), with
 * noiseModel::Robust over it when loss != VF_LOSS_NONE -- the absolute pose GraphManager::addBetweenFactor takes as poseEstimate and
 * discards.  Z = (q_wxyz, t) and p live in the graph's WORLD frame (the frame of vf_set_initial_state): lever arms and the alignment of
 * the sensor's datum with it are the caller's.  cov36 in tangent order [rot, trans]; cov9 row-major.
 * The factor is staged like a between factor and applied at vf_solve; a fix for a key already solved and still resident is written
 * at the next solve, as late band odometry is.  It takes the key's band slot (one factor per slot): the key must carry no band between
 * factor, staged or resident, else VF_ERR_CAPACITY with nothing staged -- reserve a node of its own for a fix (vf_reserve_node at its
 * stamp), as every sensor measurement of the reference does; such a key has an IMU factor and no odometry ending at it.  A later
 * vf_add_between ending at the key becomes a far factor by the rule that holds for a second factor on a key.  key - 1 must still be in
 * the window (VF_ERR_BAD_KEY; the oldest keyframe and key 0 cannot take one), also at the solve that applies it (dropped as late
 * odometry is, and reported by that vf_solve).
 * The factor is absorbed into the marginal prior when keyframe key - 1 is marginalised -- one update earlier than a unary factor
 * strictly must be -- at its linearisation of that moment; a handle that drops instead of marginalising drops it at that moment.
 * vf_graph_get_staged reports it as kind 4 (pose) or 5 (position) with key1 = key2 = key (a position's covariance in the translation
 * block of cov36), vf_graph_get_staged_loss its loss; vf_get_factor_errors returns btw_prev_key = key for its slot: a factor on ONE
 * key.  vf_get_consistency counts it in class VF_FACTOR_BETWEEN, so a position fix's 3 rows are judged against the 6-row threshold.
 * VF_ERR_INVALID: a loss id outside 0..3, k not finite or <= 0, a null pointer, a rotation that is no quaternion; VF_ERR_NOT_SPD:
 * the covariance. */
int vf_add_absolute_pose(vf_graph* g, uint64_t key, const double q_wxyz[4], const double t[3], const double cov36[36], int loss, double k);
int vf_add_absolute_position(vf_graph* g, uint64_t key, const double p[3], const double cov9[9], int loss, double k);
/* the kinds (VF_ABSOLUTE_*) of the factors in the band slots of the solved keys key0 .. key0+n-1, as the last vf_solve left them */
int vf_get_absolute_factors(vf_graph* g, uint64_t key0, int n, int32_t* kind);
/* GraphManager::addFactor(const CombinedImuFactor&) (GraphManager.cpp:90-94): queue a READY-MADE preintegrated factor
 * X(key-1),V(key-1),X(key),V(key),B(key-1),B(key) as its 190-double record (layout at the top of this file; e.g. what
 * vf_get_imu_factor returns) instead of cutting one from the IMU buffer.  key must be the next key (current + 1); the
 * node time advances by the record's deltaTij. */
int vf_add_imu_factor(vf_graph* g, uint64_t key, const double* rec190);
/* GraphManager::solve (GraphManager.cpp:101-141).  With a fixed lag, a between factor (band or far) added after its older
 * key has left the window is late odometry: the solve drops it, returns VF_ERR_BAD_KEY once, gives everything else it had
 * taken back to the queues, and the next vf_solve runs on the rest. */
int vf_solve(vf_graph* g);
/* GraphManager::getState / getBias / getMostRecentPoseTime (GraphManager.cpp:164-178, 71-75) */
int vf_get_state(vf_graph* g, double q[4], double t[3], double v[3], double bias[6]);
int vf_get_bias(vf_graph* g, double bias[6]);
int vf_most_recent_pose_time(vf_graph* g, double* time, uint64_t* key);
/* GraphManager::getMostRecentEstimate (GraphManager.cpp:77-81).  The reference never assigns the member it returns
 * (_mostRecentEstimate, GraphManager.h:109), so this is the default NavState -- identity pose, zero velocity -- always;
 * use vf_get_state for the estimate. */
int vf_get_most_recent_estimate(vf_graph* g, double q[4], double t[3], double v[3]);
/* GraphManager::addOptimizationCallback (GraphManager.cpp:96-99) */
int vf_set_callback(vf_graph* g, vf_callback cb, void* user);
/* ISAM2::marginalCovariance(X(key)) (no reference call: the reference never asks for it) -- the 15x15 marginal covariance of a
 * solved key (tangent order [omega, v] of Pose3, velocity, bias [acc, gyro]; reference-compat handles: at the linearisation
 * points, as iSAM2 factors it).  The first call after a solve computes the window's covariances (vf_engine_marginals), later ones
 * read them; vf_solve and vf_set_initial_state void them.  VF_ERR_INVALID before the first solve and, unless
 * vf_graph_opts.far_covariance is set, while far factors are alive;
 * VF_ERR_BAD_KEY for a key not solved yet or marginalised out of the window.  Takes the state lock like vf_get_state: never call it
 * from inside a callback. */
int vf_get_marginal_covariance(vf_graph* g, uint64_t key, double cov225[225]);
/* Degeneracy scores of the fused estimate itself: `metric` on the subsets of subset_mask of the nav_msgs pose covariance
 * (VF_SCORE_COVARIANCE) or information (VF_SCORE_INFORMATION) of keys key0 .. key0+n-1, the window as one time series (the score of
 * its oldest key is 0).  out: popcount(subset_mask) rows of n values, in ascending subset id.  If the last solve has no covariances
 * yet they are computed with VF_MARGINALS_POSE (and VF_MARGINALS_FAR under vf_graph_opts.far_covariance), then the scores
 * (vf_engine_marginal_scores); vf_solve and vf_set_initial_state void them.  Refusals and lock rule as vf_get_marginal_covariance. */
int vf_get_degeneracy_scores(vf_graph* g, int source, int metric, unsigned subset_mask, uint64_t key0, int n, double* out);
/* factor->error(values) of the factors of the last solve (vf_engine_factor_errors; reference-compat handles: at the linearisation
 * points): for keys key0 .. key0+n-1 the error 0.5 |r|^2 of the IMU factor X(key-1) -> X(key) and of the band between factor ending
 * at the key (-1: none), and the key that between factor starts from (UINT64_MAX: none).  Any output may be NULL.  The first call
 * after a solve computes, from the residuals the solve left, later ones read; vf_solve and vf_set_initial_state void the result.
 * A vf_reserve_node in between changes nothing.  Loop closures (far factors) are not keyed by their end: their errors are read
 * through the engine call, vf_engine_read_far_errors; they are part of vf_get_consistency.  VF_ERR_INVALID before the first solve;
 * VF_ERR_BAD_KEY for a key not solved yet or gone from the window.  Takes the state lock: never call it from inside a callback. */
int vf_get_factor_errors(vf_graph* g, uint64_t key0, int n, double* imu_err, double* btw_err, uint64_t* btw_prev_key);
/* ... and the nonlinear far factors (loop closures) alive after the last solve, in the order of the engine's list: *n of them, for
 * each its two keys, its loss (VF_LOSS_*) with its parameter k, and its error (rho(s) under a loss: vf_engine_read_far_errors).  The
 * arrays hold VF_MAX_FAR_LIMIT entries; any of them may be NULL.  Refusals and lock rule as vf_get_factor_errors. */
int vf_get_far_factors(vf_graph* g, int* n, uint64_t* prev_key, uint64_t* cur_key, int* loss, double* k, double* err);
/* graph.error(values) and printErrors with a threshold: the window's summary by factor class (vf_consistency; argmax in keyframe
 * slots of the handle's engine).  chi2_threshold6 as in vf_engine_factor_errors; a call with thresholds computes again (the
 * errors are the same bits), one without reads what the last call since the solve left, its flags included.  Refusals and lock rule as vf_get_factor_errors. */
int vf_get_consistency(vf_graph* g, const double* chi2_threshold6, vf_consistency* out);
/* The state at `time`, between two solves: predicted from the last solved key through the steps of every queued, not yet solved
 * IMU factor and then what vf_reserve_node(time) would cut from the IMU buffer at this moment -- which is not consumed
 * (vf_engine_propagate_tail; reference_compat handles predict from the estimate).  cov225 (may be NULL): the propagated covariance,
 * tangent order of vf_get_marginal_covariance; if the last solve has no covariances yet they are computed first, as
 * vf_get_marginal_covariance does (vf_graph_opts.far_covariance is honoured, its refusals apply).  `time` equal to the last key's time
 * with nothing queued gives the solved state and its marginal.  VF_ERR_INVALID: before the first successful solve; a queued factor
 * is a ready-made record (vf_add_imu_factor); `time` precedes the last reserved key's time.  Takes the graph, buffer and state
 * locks in vf_reserve_node's order: never call it from inside a callback. */
int vf_predict_state(vf_graph* g, double time, double q[4], double t[3], double v[3], double bias[6], double cov225[225]);
/* The innovation test of an odometry increment BEFORE vf_add_between takes it (vf_engine_gate_tail on the handle's window; its
 * comment has the quantity, the reach and the 6-dof quantiles a caller is likely to pass: 16.81 at 99 %, 22.46 at 99.9 %).  q, t,
 * cov36: what vf_add_between would be given -- the record is built and validated by the same routine, with the same error codes.
 * cur_key: a reserved key in [solved key, current key]; the IMU steps are those of the queued, not yet solved factors up to
 * cur_key, concatenated as vf_predict_state does, nothing is cut from the IMU buffer; cur_key = the solved key means no steps.
 * prev_key: the last solved key or the one before it, still in the window -- anything else returns VF_OK with status
 * VF_GATE_OUT_OF_REACH (two solved keys any distance apart: vf_gate_closure below).  If the last solve has no covariances yet they are computed first: VF_MARGINALS_TAIL while no far factor is
 * alive (vf_get_marginal_covariance, the scores and the covariance callbacks compute the full ones when they are asked), otherwise
 * as vf_predict_state does, vf_graph_opts.far_covariance honoured and its refusals applied.  reference_compat handles gate from
 * the estimate.  Nothing is consumed or staged: vf_add_between + vf_solve after a gate give the bits of a handle that never gated.
 * Between factors of other sensors that are staged but not solved yet are not part of the prediction.  Locks and refusals as
 * vf_predict_state (never from inside a callback); VF_ERR_BAD_KEY also for keys not reserved in order or a cur_key solved already. */
int vf_gate_between(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q[4], const double t[3], const double cov36[36],
                    double chi2_threshold, vf_gate_result* out);
/* The same test of a LOOP CLOSURE before vf_add_between takes it: a between factor on two solved keys of the window, any distance
 * apart (vf_engine_gate_closures on the handle's window; its comment has the quantity).  q, t, cov36: what vf_add_between would be
 * given -- the record is built and validated by the same routine, with the same error codes.  Both keys must be solved and still in
 * the window: anything else returns VF_OK with status VF_GATE_OUT_OF_REACH (an end that is reserved but not solved yet is
 * vf_gate_between's to test).  Far factors alive -- the closures already made -- are ALWAYS part of the covariance, whatever
 * vf_graph_opts.far_covariance says: a loop-closure gate that ignores the closures already made has no meaning.  The covariances
 * the handle keeps (vf_get_marginal_covariance, vf_gate_between) are neither used nor voided.  reference_compat handles gate from
 * the estimate (VF_GATE_FROM_ESTIMATE: both ends are solved keys, so both poses are the estimate's).  Nothing is consumed or staged: vf_add_between + vf_solve
 * after a gate give the bits of a handle that never gated.  out->a, out->b: the keys' slots in the window.  joint_cov144: the 12 x 12
 * joint covariance of the two poses (prev_key first), or NULL.  Locks and refusals as vf_gate_between: never call it from inside a
 * callback. */
int vf_gate_closure(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q[4], const double t[3], const double cov36[36],
                    double chi2_threshold, vf_closure_gate_result* out, double* joint_cov144);
/* the callback of vf_set_callback plus the marginal covariance of the solved keyframe */
typedef void (*vf_cov_callback)(void* user, double time, const double q[4], const double t[3], const double v[3],
                                const double bias[6], const double cov225[225]);
/* Only while one is registered does vf_solve compute covariances: after the result read, before the callbacks (which run inside the
 * state lock as the plain ones do).  If they cannot be had (far factors alive without vf_graph_opts.far_covariance, undamped system
 * not positive definite) the covariance
 * callbacks receive NaN and vf_last_error says why; the solve itself succeeds. */
int vf_set_covariance_callback(vf_graph* g, vf_cov_callback cb, void* user);
/* GraphManager::graph()->size(): factors staged since the last solve (3 priors at start +
 * between factors; IMU factors wait in the queue, GraphManager.cpp:66,150) and the queue length */
int vf_graph_staged(vf_graph* g, int* staged_factors, int* queued_imu_factors);
/* GraphManager::graph() (GraphManager.h:42, GraphManager.cpp:46-49), by index 0 .. staged_factors - 1: what the reference's tests
 * read from the staged NonlinearFactorGraph (test/UnitTests.cpp:200,222-233: its size, a factor's keys, measured()).
 * kind 0 / 1 / 2: PriorFactor<Pose3> on X(0) (q, t = its mean, cov36 = diag sigma^2 in [rot, trans] order), PriorFactor<Vector3>
 * on V(0) (t = mean, top-left 3 x 3 of cov36), PriorFactor<ConstantBias> on B(0) (t = accelerometer part, q[1..3] = gyro part,
 * q[0] = 0; cov36 6 x 6) -- all three on key1 = key2 = 0, present until the first solve takes them.  kind 3: BetweenFactor<Pose3>
 * X(key1) -> X(key2), measured() = (q, t) with q normalised as gtsam::Rot3(w, x, y, z) does, cov36 as handed in.  Any output
 * pointer may be null.  VF_ERR_BAD_KEY beyond the end. */
int vf_graph_get_staged(vf_graph* g, int index, int* kind, uint64_t* key1, uint64_t* key2, double q[4], double t[3],
                        double cov36[36]);
/* ... and its loss (the companion of vf_graph_get_staged, same index): VF_LOSS_NONE and 0 for the priors and for a Gaussian factor.
 * Either output pointer may be null.  VF_ERR_BAD_KEY beyond the end. */
int vf_graph_get_staged_loss(vf_graph* g, int index, int* loss, double* k);
/* diagnostics (extra): cost after the last solve and the LM trials accepted / rejected / failed (normal equations not
 * positive definite) over the life of the handle */
int vf_graph_lm_stats(vf_graph* g, double* cost, int* accepted, int* rejected, int* solve_failures);
/* diagnostics (extra): keyframes in the window of the last solve; conjugate-gradient corrections every solve of the handle's
 * engine is now followed by (vf_engine_opts.refine_iterations: 0 until the window outgrows refine_min_keyframes -- a
 * whole-history handle, lag = 0, gets there by itself -- 12 from then on); LM trials kept provisionally so far (lm_excursion) */
int vf_graph_solver_info(vf_graph* g, int* window_keyframes, int* refine_corrections, int* provisional_trials);
/* diagnostics (extra; handles made with incremental != 0): updates so far, how many of them re-eliminated the whole history, and
 * the keys the last update's forward sweep started at / its back substitution stopped at */
int vf_graph_incremental_info(vf_graph* g, long* updates, long* whole_window_updates, uint64_t* first_eliminated_key,
                              uint64_t* last_substituted_key);
/* smoothed states of keys [key0, key0+n) after the last solve (extra; iSAM2 calculateEstimate) */
int vf_get_trajectory(vf_graph* g, uint64_t key0, int n, double* state16);
/* preintegrated record of the factor ending at `key` (extra; firstFactor->preintegratedMeasurements()) */
int vf_get_imu_factor(vf_graph* g, uint64_t key, double* rec190);

#ifdef __cplusplus
}
#endif
#endif
