// engine/engine_create.inc -- errors, option defaults (struct_size), creation from ONE device allocation, destruction.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.

const char* vf_last_error(void) { return g_err.c_str(); }
void vf_set_last_error_(const char* msg) { g_err = msg ? msg : ""; }  // used by vf_graph.cpp
const char* vf_version(void) { return "vilfusion-mi355x 0.1 (gfx950, float64)"; }

int vf_device_count(int* count) {
    if (!count) return fail(VF_ERR_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(VF_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return VF_OK;
}

#undef vf_engine_default_opts
#undef vf_engine_default_tuning
static void engine_defaults(vf_engine_opts* o) {
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(*o);
    o->windows = 1;
    o->capacity = 1088;
    o->bandwidth = 3;
    o->device = 0;
    o->gravity[0] = 0.0; o->gravity[1] = 0.0; o->gravity[2] = -9.81;
    // gtsam::LevenbergMarquardtParams defaults (the optimiser commented out at
    // GraphManager.cpp:128-129): lambdaInitial 1e-5, lambdaFactor 10
    o->lambda0 = 1e-5; o->lambda_up = 10.0; o->lambda_down = 10.0;
    o->lambda_min = 1e-12; o->lambda_max = 1e10;
    o->cold_start = 0;
    o->accept_rel = 1e-9;
    o->refine_iterations = -1;       // auto: windows longer than refine_min_keyframes
    o->refine_min_keyframes = 1536;
    o->refine_rel_stop = 1e-8;
    o->lm_excursion = -1;            // auto: 3 on engines that refine, classical LM otherwise
    o->gauge_floor = 3e-4;
    o->incremental = 0;
    o->wildfire = 0.0;
    o->min_model_fidelity = 0.0;
    o->max_far_factors = 0;          // = VF_MAX_EXTRA
}
static void tuning_defaults(vf_engine_tuning* t) {
    memset(t, 0, sizeof(*t));
    t->struct_size = (uint32_t)sizeof(*t);
    t->sweep_two_sided_max = 256;
    t->hybrid_threshold = 256;   // partitioned form: 0.0095 ms per window; the sweep: 2.9 ms whatever their number
    t->use_hip_graph = 0;
    t->solve_split_min = 2048;
    t->solve_assemble_min = 768;
    t->solve_assemble_waves = 2;
    t->hybrid_active_list = 1;
    t->far_batch_columns = 1;
    t->far_big_forms = 0;
    t->solve_backsub_form = 0;   // by batch: the one-per-SIMD form up to one window per SIMD
}
// The caller's struct may be shorter than the library's (built against an older header): only its own bytes are written, and
// struct_size says how many those are.  A struct the library does not know (longer than its own) gets the bytes it does know.
void vf_engine_default_opts_sized(vf_engine_opts* o, uint32_t struct_size) {
    if (!o || struct_size < sizeof(uint32_t)) return;
    vf_engine_opts full;
    engine_defaults(&full);
    const uint32_t n = struct_size < sizeof(full) ? struct_size : (uint32_t)sizeof(full);
    memcpy(o, &full, n);
    o->struct_size = n;
}
void vf_engine_default_opts(vf_engine_opts* o) { vf_engine_default_opts_sized(o, (uint32_t)sizeof(vf_engine_opts)); }
void vf_engine_default_tuning_sized(vf_engine_tuning* t, uint32_t struct_size) {
    if (!t || struct_size < sizeof(uint32_t)) return;
    vf_engine_tuning full;
    tuning_defaults(&full);
    const uint32_t n = struct_size < sizeof(full) ? struct_size : (uint32_t)sizeof(full);
    memcpy(t, &full, n);
    t->struct_size = n;
}
void vf_engine_default_tuning(vf_engine_tuning* t) { vf_engine_default_tuning_sized(t, (uint32_t)sizeof(vf_engine_tuning)); }

int vf_engine_create(const vf_engine_opts* o, vf_engine** out) { return vf_engine_create_tuned(o, nullptr, out); }
// on_stream: the engine works on a stream somebody else owns (the column engine of a handle's far factors, the engine a growing
// handle moves into) -- hipStreamCreate costs 9 ms on this stack (the HSA queue behind it), more than everything else here together
// form_windows: the batch size the K4 form is chosen for when it is not the engine's own (a column engine solves its parent's
// window, in its parent's form, however many columns there are)
static int create_engine(const vf_engine_opts* o_in, const vf_engine_tuning* t_in, bool on_stream, hipStream_t given, vf_engine** out, int form_windows = 0);
int vf_engine_create_tuned(const vf_engine_opts* o_in, const vf_engine_tuning* t_in, vf_engine** out) {
    return create_engine(o_in, t_in, false, nullptr, out);
}
static int create_engine(const vf_engine_opts* o_in, const vf_engine_tuning* t_in, bool on_stream, hipStream_t given, vf_engine** out, int form_windows) {
    if (!o_in || !out) return fail(VF_ERR_INVALID, "null argument");
    // the structs as THIS library knows them: the caller's bytes over the defaults
    vf_engine_opts o_full;
    vf_engine_tuning t_full;
    engine_defaults(&o_full);
    tuning_defaults(&t_full);
    if (o_in->struct_size < 8 || o_in->struct_size > sizeof(o_full))
        return fail(VF_ERR_INVALID, "vf_engine_opts.struct_size = %u: this library knows sizes up to %zu (fill the struct with vf_engine_default_opts; "
                    "a caller built against a newer header needs a newer library)", o_in->struct_size, sizeof(o_full));
    memcpy(&o_full, o_in, o_in->struct_size);
    o_full.struct_size = (uint32_t)sizeof(o_full);
    if (t_in) {
        if (t_in->struct_size < 8 || t_in->struct_size > sizeof(t_full))
            return fail(VF_ERR_INVALID, "vf_engine_tuning.struct_size = %u: this library knows sizes up to %zu", t_in->struct_size, sizeof(t_full));
        memcpy(&t_full, t_in, t_in->struct_size);
        t_full.struct_size = (uint32_t)sizeof(t_full);
    }
    const vf_engine_opts* o = &o_full;
    const vf_engine_tuning* t = &t_full;
    if (o->windows < 1 || o->capacity < 2) return fail(VF_ERR_INVALID, "windows >= 1 and capacity >= 2 required");
    if (o->bandwidth < 1 || o->bandwidth > VF_MAX_BANDWIDTH)
        return fail(VF_ERR_INVALID, "bandwidth must be in 1..%d", VF_MAX_BANDWIDTH);
    if (o->chunks < 0 || o->chunks > 4096) return fail(VF_ERR_INVALID, "chunks must be in 0..4096");
    if (o->max_far_factors < 0 || o->max_far_factors > VF_MAX_FAR_LIMIT) return fail(VF_ERR_INVALID, "max_far_factors must be in 0..%d", VF_MAX_FAR_LIMIT);
    if (!(o->accept_rel >= 0.0) || !(o->accept_rel < 1.0)) return fail(VF_ERR_INVALID, "accept_rel must be in [0, 1)");
    if (o->refine_iterations < -1 || o->refine_iterations > 64) return fail(VF_ERR_INVALID, "refine_iterations must be in -1..64");
    if (!(o->gauge_floor >= 0.0) || !(o->gauge_floor < 1e6)) return fail(VF_ERR_INVALID, "gauge_floor must be in [0, 1e6)");
    if (o->lm_excursion < -1 || o->lm_excursion > 16) return fail(VF_ERR_INVALID, "lm_excursion must be in -1..16");
    if (!(o->refine_rel_stop >= 0.0) || !(o->refine_rel_stop < 1.0)) return fail(VF_ERR_INVALID, "refine_rel_stop must be in [0, 1)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VF_ERR_NO_DEVICE, "no HIP device visible; libvilfusion has no CPU path");
    if (o->device < 0 || o->device >= ndev) return fail(VF_ERR_INVALID, "device %d out of range (%d)", o->device, ndev);
    HIPCHK(hipSetDevice(o->device));
    vf_engine* e = new vf_engine();
    e->opts = *o;
    e->tune = *t;
    e->x_cap = o->max_far_factors > 0 ? o->max_far_factors : VF_MAX_EXTRA;
    vf::View& v = e->v;
    v.B = o->windows;
    v.M = (o->capacity + 63) / 64 * 64;
    v.G = (long)v.B * v.M;
    for (int i = 0; i < 3; i++) v.grav[i] = o->gravity[i];
    v.lam_up = o->lambda_up; v.lam_down = o->lambda_down; v.lam_min = o->lambda_min; v.lam_max = o->lambda_max;
    v.accept_rel = o->accept_rel;
    v.split_min = t->solve_split_min > 0 ? t->solve_split_min : 0;
    v.asm_min = t->solve_assemble_min > 0 ? t->solve_assemble_min : 0;
    v.asm_waves = t->solve_assemble_waves == 1 ? 1 : 2;
    v.bwd_form = t->solve_backsub_form == 1 || t->solve_backsub_form == 2 ? t->solve_backsub_form : 0;
    {
        // the SIMDs of the device (four per compute unit), read once, here: the batch up to which the back substitution has a SIMD
        // per window (0 = not known: the two-per-SIMD form at every batch)
        int cus = 0;
        v.simds = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o->device) == hipSuccess && cus > 0 ? 4 * cus : 0;
    }
    if (on_stream) { e->stream = given; e->own_stream = false; }
    else HIPCHK(hipStreamCreate(&e->stream));
    HIPCHK(e->ev0.ensure());
    HIPCHK(e->ev1.ensure());
    const size_t G = (size_t)v.G, tiles = G / 64;
    int rc = VF_OK;
    {
        // everything the AL() lines below ask for, plus slack for their 256-byte alignment (alloc() falls back to allocations of
        // its own if this estimate is ever short)
        const size_t P0 = o->chunks >= 2 ? (size_t)o->chunks : (o->chunks == 0 && (form_windows > 0 ? form_windows : o->windows) <= 128 ? 96 : 0);
        size_t dbl = G * (32 + vf::HROW + 15 + 15 + vf::PANEL) + tiles * 64 * (vf::IMU_IN + 2 * vf::IMU_R + vf::BTW_IN + 2 * vf::BTW_OUT) +
                     2 * (G / vf::JT) * vf::JT_STRIDE + 64 + (size_t)v.B * (vf::PRIOR_IN + 2 * vf::PRIOR_OUT + 48 + 729 + 27 + 56 + 8) + vf::HROW + vf::PLACE_CELLS;
        if (P0 >= 2) dbl += G * vf::VROW + (size_t)v.B * P0 * (vf::SEPK + vf::SEPL);
        if (o->incremental) dbl += (G >> vf::CK_LOG) * vf::CK_SZ;
        const size_t ints = G + 16 * (size_t)v.B + 64;
        if ((rc = e->reserve(dbl * sizeof(double) + ints * sizeof(int) + 64 * 256)) != VF_OK) { vf_engine_destroy(e); return rc; }
    }
#define AL(p, n) if ((rc = e->alloc(&(p), (n))) != VF_OK) { vf_engine_destroy(e); return rc; }
    AL(v.x, 2 * 16 * G);
    AL(v.imu_in, tiles * vf::IMU_IN * 64);
    AL(v.imu_r, 2 * tiles * vf::IMU_R * 64);
    AL(v.imu_j, 2 * (G / vf::JT) * vf::JT_STRIDE);
    AL(v.btw_a, G);
    AL(v.btw_in, tiles * vf::BTW_IN * 64);
    AL(v.btw_out, 2 * tiles * vf::BTW_OUT * 64);
    AL(v.prior_k, (size_t)v.B);
    AL(v.prior_in, (size_t)v.B * vf::PRIOR_IN);
    AL(v.prior_out, 2 * (size_t)v.B * vf::PRIOR_OUT);
    AL(v.mp_on, (size_t)v.B);
    AL(v.mp_x, (size_t)v.B * 48);
    AL(v.mp_L, (size_t)v.B * 729);
    AL(v.mp_eta, (size_t)v.B * 27);
    AL(v.mp_out, 2 * (size_t)v.B * 28);
    // K4 form: chunks = 0 picks it from the batch size: up to 128 windows -> partitioned solve with at most 96 chunks,
    // fewer on short windows (latency form); more windows -> one sweep per window (throughput form; the partitioned
    // solve does about twice the arithmetic).  1 forces sweeps.
    v.P = o->chunks >= 2 ? o->chunks : (o->chunks == 0 && (form_windows > 0 ? form_windows : o->windows) <= 128 ? 96 : 0);
    v.P_fit = o->chunks == 0 ? 1 : 0;
    // (the chunk kernels launch windows x P workgroups: no more chunks than a full window could use)
    if (v.P_fit && v.P) v.P = vf::chunk_count(v.M, v.P, 1);
    if (v.P < 2) v.P = 0;
    AL(v.H, G * vf::HROW);
    AL(v.gvec, G * 15 + 64); // + slack: the solver's row fetch reads 64 lanes of a 15-double row (the excess is never used)
    AL(v.place, vf::PLACE_CELLS);
    AL(v.zrow, vf::HROW);         // a block row of zeros: what the solver fetches for rows outside the window
    AL(v.delta, G * 15 + (size_t)v.B);   // + one solve-failure flag per window (time-sharded windows: reduced with the increments)
    AL(v.Lp, G * vf::PANEL);
    if (v.P) {
        const size_t BP = (size_t)v.B * v.P;
        AL(v.Vp, G * vf::VROW);
        AL(v.sepR, BP * vf::SEPK);       // one buffer, slots of [sepR | sepS | sepC] (vf_kernels.hpp "SEPK")
        v.sepS = v.sepR + vf::SEPM;
        v.sepC = v.sepR + 2 * vf::SEPM;
        AL(v.sepL, BP * vf::SEPL);
    }
    AL(v.lo, (size_t)v.B);
    AL(v.hi, (size_t)v.B);
    AL(v.sel, (size_t)v.B);
    AL(v.fail, (size_t)v.B);
    AL(v.fresh, (size_t)v.B);
    AL(v.lambda, (size_t)v.B);
    AL(v.cost, (size_t)v.B);
    AL(v.n_acc, (size_t)v.B);
    AL(v.n_rej, (size_t)v.B);
    AL(v.n_fail, (size_t)v.B);
    AL(v.done, (size_t)v.B);
    AL(v.n_active, 4);
    v.gate = 0;
    v.gate_T = t->hybrid_threshold;
    v.tw_max = t->sweep_two_sided_max;
    v.stop_on = 0;
    v.rel_tol = v.abs_tol = 0.0;
    v.sh_r = 0;
    v.sh_G = 1;
    v.gauge_floor = o->gauge_floor;
    v.sh_all_jac = 0;         // set at every linearisation: 1 while the engine refines (the refined solve applies J on whole increments)
    v.wildfire = o->wildfire >= 0.0 ? o->wildfire : 0.0;
    v.min_fidelity = o->min_model_fidelity > 0.0 ? o->min_model_fidelity : 0.0;
    if (v.min_fidelity > 0.0) { AL(v.model, (size_t)v.B); }
    if (o->incremental) {
        AL(v.inc_k, (size_t)v.B);
        AL(v.inc_stop, (size_t)v.B);
        AL(v.inc_from, (size_t)v.B);
        AL(v.ck, (G >> vf::CK_LOG) * vf::CK_SZ);
        HIPCHK(hipMemsetAsync(v.inc_k, 0x7f, v.B * sizeof(int), e->stream));
    }
    AL(e->lambda0_dev, (size_t)v.B);
    AL(e->sigma_dev, 16);
    AL(e->status_dev, 4);
#undef AL
    HIPCHK(hipMemsetAsync(v.btw_a, 0xff, G * sizeof(int), e->stream));   // -1 = empty slot
    HIPCHK(hipMemsetAsync(v.prior_k, 0xff, v.B * sizeof(int), e->stream));
    std::vector<double> lam((size_t)v.B, o->lambda0);
    HIPCHK(hipMemcpyAsync(v.lambda, lam.data(), v.B * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->lambda0_dev, lam.data(), v.B * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // measured on MI355X (ROCm 7.0, one 1000-pose window, K = 5): 2.99 ms replayed from the graph vs 2.91 ms
    // with plain asynchronous launches -- the queue is never empty, so there is no launch gap to remove.
    // Hence opt-in only.
    e->graph_off = t->use_hip_graph == 0;
    e->mem.one_window = v.B == 1;
    e->mem.no_warm = o->cold_start != 0;
    e->mem.incremental = o->incremental != 0;
    HIPCHK(hipStreamSynchronize(e->stream));
    e->h_lo.assign(v.B, 0);
    e->h_hi.assign(v.B, 0);
    *out = e;
    return VF_OK;
}

void vf_engine_destroy(vf_engine* e) {
    Entry entry_(e, Entry::reads);
    if (!e) return;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    e->drop_graph();
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->far_columns) { vf_engine_destroy(e->far_columns); e->far_columns = nullptr; }
    if (e->stream2) { (void)hipStreamSynchronize(e->stream2); (void)hipStreamDestroy(e->stream2); }
    if (e->stream && e->own_stream) (void)hipStreamDestroy(e->stream);
    delete e;      // (frees what owns itself, buffers and events, vf_device_buf.hpp, while entry_ still holds the engine's device current)
}
