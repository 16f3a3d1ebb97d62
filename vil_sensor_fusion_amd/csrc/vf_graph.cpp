// vf_graph.cpp -- host-side mirror of VILFusion::GraphManager + VILFusion::IMUManager behind the
// C ABI (include/vilfusion.h "GraphManager surface").
//
// Only bookkeeping lives here: key numbering, the IMU sample deque and how IMUManager::getFactor
// cuts it (which samples are dropped / integrated / interpolated), the queue of not-yet-added
// IMU factors, staged between factors, the two mutexes and the callbacks.  Every number that
// depends on the factor math -- preintegration (K0), initial-value prediction, linearisation,
// the LM solve -- is computed by the HIP engine; there is no CPU fallback.
//
// Reference: gtsam_fusion/src/gtsam_fusion/GraphManager.cpp, IMUManager.cpp.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

namespace {

struct LateFactor { bool any = false; uint64_t a = 0, b = 0; };   // the first between factor a solve has dropped as late odometry
// what one vf_solve took from the handle (take), as its steps have left it, and what they decided (give_back, publish_far_list)
struct SolveTake {
    std::deque<PendingImu> imus;
    std::vector<PendingBetween> betweens, fars;
    size_t fars_snapshot = 0;               // length of the handle's far list when `fars` was copied: what is behind it was added since
    int staged = 0, far_new = 0;            // the handle's counts, less what was dropped as late
    std::vector<StagedFactor> log;
    bool priors = false, marginalised = false;   // (marginalised: this solve has moved the window's oldest key)
    uint64_t last_key = 0;
    double last_time = 0.0;
    LateFactor late_far, late_band;         // dropped: a far factor that was late when the solve began; a band factor (its end key is to be unmarked)
    bool fars_changed = false;              // `fars` is no longer what the handle's list holds
    bool requeue = false;                   // the solve failed before the optimisation: everything goes back
    vf_between_loss_setter set_loss = nullptr;   // the handle's set_between_loss as it stood at the take (read under graph_mutex, where it is written)
    vf_far_robust_setter set_far_robust = nullptr;   // ... and its two calls for the losses of far factors, likewise
    vf_far_loss_getter get_far_loss = nullptr;
    vf_absolute_setter set_absolute = nullptr;   // ... and the one for absolute factors
};

struct Lap {   // VF_SOLVE_TIMING: "[vf_solve] <label> <us>" on stderr behind every step of a solve (tools/gm_lap_summary.py reads the labels)
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        static const bool timing = getenv("VF_SOLVE_TIMING") != nullptr;
        const auto now = timing ? std::chrono::steady_clock::now() : last;
        if (timing) fprintf(stderr, "[vf_solve] %-12s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - last).count());
        last = now;
    }
};

// R upper-triangular, R^T R = cov^-1 (noiseModel::Gaussian::Covariance, SensorManagerRos.cpp:99).
// 6x6 noise-model construction is factor *construction*, done once per measurement on the host
// exactly where the reference does it.
bool sqrt_info_upper6(const double* cov, double* Rp) {
    // reverse Cholesky cov = U U^T (U upper) then R = U^-1
    double U[36] = {0}, T[36] = {0};
    for (int j = 5; j >= 0; j--) {
        double d = cov[j * 6 + j];
        for (int l = j + 1; l < 6; l++) d -= U[j * 6 + l] * U[j * 6 + l];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ujj = std::sqrt(d);
        U[j * 6 + j] = ujj;
        for (int i = 0; i < j; i++) {
            double a = 0.5 * (cov[i * 6 + j] + cov[j * 6 + i]);
            for (int l = j + 1; l < 6; l++) a -= U[i * 6 + l] * U[j * 6 + l];
            U[i * 6 + j] = a / ujj;
        }
    }
    for (int c = 0; c < 6; c++) {
        T[c * 6 + c] = 1.0 / U[c * 6 + c];
        for (int r = c - 1; r >= 0; r--) {
            double a = 0.0;
            for (int l = r + 1; l <= c; l++) a += U[r * 6 + l] * T[l * 6 + c];
            T[r * 6 + c] = -a / U[r * 6 + r];
        }
    }
    int o = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) Rp[o++] = T[r * 6 + c];
    return true;
}

}  // namespace

extern "C" {

// defined in vf_engine.hip: graph-level messages go to the same thread-local vf_last_error()
void vf_set_last_error_(const char* msg);

static int gerr(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

#undef vf_graph_default_opts
#undef vf_engine_default_opts
static void graph_defaults(vf_graph_opts* o) {
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(*o);
    o->capacity = 4096;
    o->lag = 0;
    o->iterations = 5;
    o->device = 0;
    // GraphManager.cpp:27-31: rad,rad,rad,m,m,m ; m/s ; bias
    const double s[15] = {1e-6, 1e-6, 1e-6, 5e-5, 5e-5, 5e-5, 1e-5, 1e-5, 1e-5, 1e-7, 1e-7, 1e-7, 1e-7, 1e-7, 1e-7};
    memcpy(o->prior_sigma, s, sizeof(s));
    o->rel_tol = 1e-5;   // gtsam::LevenbergMarquardtParams relativeErrorTol / absoluteErrorTol
    o->abs_tol = 1e-5;
    o->cold_start = 0;
    o->fixed_capacity = 0;
    o->reference_compat = 0;
    o->relin_threshold = 1e-4;   // GraphManager.cpp:40
    o->incremental = 0;
    o->wildfire = 0.0;
    o->min_model_fidelity = 0.0;
    o->synchronous_staging = 0;
    o->max_far_factors = 0;      // = VF_MAX_FAR_LIMIT
    o->far_covariance = 0;
}
// (the caller's struct may be shorter than the library's: include/vilfusion.h "struct_size")
void vf_graph_default_opts_sized(vf_graph_opts* o, uint32_t struct_size) {
    if (!o || struct_size < sizeof(uint32_t)) return;
    vf_graph_opts full;
    graph_defaults(&full);
    const uint32_t n = struct_size < sizeof(full) ? struct_size : (uint32_t)sizeof(full);
    memcpy(o, &full, n);
    o->struct_size = n;
}
void vf_graph_default_opts(vf_graph_opts* o) { vf_graph_default_opts_sized(o, (uint32_t)sizeof(vf_graph_opts)); }

int vf_create(const vf_imu_params* imu, const vf_graph_opts* opts, vf_graph** out) {
    if (!imu || !out) return gerr(VF_ERR_INVALID, "null argument");
    vf_graph_opts o;
    graph_defaults(&o);
    if (opts) {
        if (opts->struct_size < 8 || opts->struct_size > sizeof(o))
            return gerr(VF_ERR_INVALID, "vf_graph_opts.struct_size = %u: this library knows sizes up to %zu (fill the struct with vf_graph_default_opts; "
                        "a caller built against a newer header needs a newer library)", opts->struct_size, sizeof(o));
        memcpy(&o, opts, opts->struct_size);
        o.struct_size = (uint32_t)sizeof(o);
    }
    if (o.capacity < 8 || o.iterations < 0 || o.lag < 0) return gerr(VF_ERR_INVALID, "bad graph options");
    if (o.lag != 0 && o.lag < 4) return gerr(VF_ERR_INVALID, "lag must be 0 or >= 4 keyframes");
    if (!(o.rel_tol >= 0.0) || !(o.abs_tol >= 0.0)) return gerr(VF_ERR_INVALID, "tolerances must be >= 0");
    if (o.reference_compat && o.lag != 0) return gerr(VF_ERR_INVALID, "reference_compat needs lag == 0 (the reference's graph is unbounded)");
    if (o.reference_compat && !(o.relin_threshold >= 0.0)) return gerr(VF_ERR_INVALID, "relin_threshold must be >= 0");
    if (o.incremental && !o.reference_compat) return gerr(VF_ERR_INVALID, "incremental needs reference_compat (the update it makes incremental is the iSAM2-like one)");
    if (o.incremental && !(o.wildfire >= 0.0)) return gerr(VF_ERR_INVALID, "wildfire must be >= 0");
    if (o.max_far_factors < 0 || o.max_far_factors > VF_MAX_FAR_LIMIT) return gerr(VF_ERR_INVALID, "max_far_factors must be in 0..%d", VF_MAX_FAR_LIMIT);
    // (a handle takes what the library can hold: while eight or fewer are alive the solver's forms are those of an engine made for
    // eight, whatever the capacity; the lists are allocated when the first far factor arrives)
    if (o.max_far_factors == 0) o.max_far_factors = VF_MAX_FAR_LIMIT;
    const double covs[6] = {imu->acc_cov, imu->gyro_cov, imu->integration_cov, imu->bias_acc_cov, imu->bias_omega_cov, imu->bias_acc_omega_int};
    for (double c : covs)
        if (!(c > 0.0) || !std::isfinite(c)) return gerr(VF_ERR_NOT_SPD, "IMU covariances must be finite and > 0");
    // the engine allocates keyframe slots in whole AoSoA tiles of 64: keep the number the growth / compaction / capacity
    // checks below work with equal to what the engine really has (a handle created with capacity 16 has 64 slots; growing
    // it "to 32" would ask vf_engine_grow for the 64 it already has)
    o.capacity = (o.capacity + 63) / 64 * 64;
    vf_engine_opts eo;
    vf_engine_default_opts(&eo);
    eo.windows = 1;
    eo.capacity = o.capacity;
    eo.device = o.device;
    eo.cold_start = o.cold_start;
    eo.min_model_fidelity = o.min_model_fidelity > 0.0 ? o.min_model_fidelity : 0.0;
    eo.max_far_factors = o.max_far_factors;
    if (o.incremental) {
        // (the refined solve corrects a whole-window factorisation through J; the incremental update keeps the panels of an
        // elimination that ran forward in time from the anchor prior -- every pivot block is the conditional information of a
        // keyframe given its past, well conditioned whatever the history's length -- and does without)
        eo.incremental = o.incremental == 2 ? 2 : 1;
        eo.wildfire = o.wildfire;
        eo.refine_iterations = 0;
        eo.lm_excursion = 0;
    }
    vf_engine* eng = nullptr;
    int rc = vf_engine_create(&eo, &eng);
    if (rc) return rc;
    vf_graph* g = new vf_graph();
    g->eng = eng;
    g->opts = o;
    g->imu = *imu;
    g->key_time.push_back(-1.0);
    // X(0)=identity, V(0)=0, B(0)=0 with the three priors (GraphManager.cpp:20-35)
    double rec[VF_PRIOR_RECORD] = {0};
    rec[0] = 1.0;
    memcpy(rec + 16, o.prior_sigma, sizeof(double) * 15);
    if ((rc = vf_engine_set_states(eng, 0, 0, 1, g->state)) || (rc = vf_engine_set_prior(eng, 0, 0, rec)) ||
        (rc = vf_engine_set_range(eng, 0, 0, 1)) || (rc = vf_engine_set_convergence(eng, o.rel_tol, o.abs_tol)) ||
        (rc = vf_engine_set_async(eng, o.synchronous_staging ? 0 : 1))) {
        vf_engine_destroy(eng);
        delete g;
        return rc;
    }
    *out = g;
    return VF_OK;
}

void vf_destroy(vf_graph* g) {
    if (!g) return;
    vf_engine_destroy(g->eng);
    delete g;
}

int vf_set_initial_state(vf_graph* g, const double state16[16]) {
    if (!g || !state16) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    std::lock_guard<std::mutex> sl(g->state_mutex);
    if (g->current_key != 0 || g->solved_key != 0) return gerr(VF_ERR_INVALID, "the initial state can only be set before the first node is reserved");
    double n = 0.0;
    for (int i = 0; i < 4; i++) n += state16[i] * state16[i];
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(state16[i])) return gerr(VF_ERR_INVALID, "initial state entry %d is not finite", i);
    if (!(n > 0.0)) return gerr(VF_ERR_INVALID, "initial rotation is not a quaternion");
    double st[16];
    memcpy(st, state16, sizeof(st));
    for (int i = 0; i < 4; i++) st[i] /= std::sqrt(n);
    double rec[VF_PRIOR_RECORD];
    memcpy(rec, st, sizeof(double) * 16);
    memcpy(rec + 16, g->opts.prior_sigma, sizeof(double) * 15);
    int rc;
    if ((rc = vf_engine_set_states(g->eng, 0, 0, 1, st)) || (rc = vf_engine_set_prior(g->eng, 0, 0, rec))) return rc;
    memcpy(g->state, st, sizeof(st));
    g->cov_valid = g->cov_tail = g->err_valid = false;
    memcpy(g->anchor, st, sizeof(st));
    return VF_OK;
}

int vf_add_imu(vf_graph* g, double time, const double acc[3], const double gyro[3]) {
    if (!g || !acc || !gyro) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->buffer_mutex);  // IMUManager.cpp:21
    ImuSample s;
    s.t = time;
    memcpy(s.acc, acc, sizeof(s.acc));
    memcpy(s.gyro, gyro, sizeof(s.gyro));
    g->buffer.push_back(s);
    return VF_OK;
}

// IMUManager::getFactor (IMUManager.cpp:27-74): which samples are dropped, integrated and
// interpolated.  The integration itself happens on the device at solve time (K0).
static void cut_imu_segment(vf_graph* g, double start, double end, std::vector<double>& steps) {
    std::lock_guard<std::mutex> lk(g->buffer_mutex);
    ImuSample prev{};
    while (!g->buffer.empty() && g->buffer.front().t <= start) {  // :35-40
        prev = g->buffer.front();
        g->buffer.pop_front();
    }
    prev.t = start;  // :44
    while (!g->buffer.empty() && g->buffer.front().t < end) {  // :46-54
        const ImuSample m = g->buffer.front();
        g->buffer.pop_front();
        const double st[7] = {m.t - prev.t, m.acc[0], m.acc[1], m.acc[2], m.gyro[0], m.gyro[1], m.gyro[2]};
        steps.insert(steps.end(), st, st + 7);
        prev = m;
    }
    if (!g->buffer.empty()) {  // :57-66, the interpolated sample stays in the buffer
        const ImuSample& f = g->buffer.front();
        const double w = (end - prev.t) / (f.t - prev.t);
        double st[7] = {end - prev.t, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 3; i++) {
            st[1 + i] = w * f.acc[i] + (1.0 - w) * prev.acc[i];
            st[4 + i] = w * f.gyro[i] + (1.0 - w) * prev.gyro[i];
        }
        steps.insert(steps.end(), st, st + 7);
    }
}

int vf_reserve_node(vf_graph* g, double time, uint64_t* key_out) {
    if (!g || !key_out) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);  // GraphManager.cpp:54
    if (g->opts.lag == 0 && g->opts.fixed_capacity && (int)(g->current_key + 1) >= g->opts.capacity)
        return gerr(VF_ERR_CAPACITY, "keyframe capacity %d exhausted (fixed_capacity; set a lag to smooth indefinitely)", g->opts.capacity);
    double start;
    if (g->current_key + 1 > 1) {
        start = g->last_pose_time;  // :59-61
    } else {
        // first node integrates from the oldest buffered sample (IMUManager.cpp:76-79)
        std::lock_guard<std::mutex> bl(g->buffer_mutex);
        if (g->buffer.empty()) return gerr(VF_ERR_INDETERMINATE, "reserveNode before any IMU measurement");
        start = g->buffer.front().t;
    }
    PendingImu p;
    p.key = g->current_key + 1;
    {
        std::lock_guard<std::mutex> sl(g->state_mutex);  // getBias(): lock order graph -> state
        memcpy(p.bias, g->state + 10, sizeof(p.bias));
    }
    cut_imu_segment(g, start, time, p.steps);
    // a factor without a single IMU step has no covariance: GTSAM would fail at the solve with the factor already in
    // the graph; here the node is refused and nothing is queued (checked before the key is consumed)
    if (p.steps.empty()) return gerr(VF_ERR_INDETERMINATE, "reserveNode(%.6f): no IMU measurement in (%.6f, %.6f]", time, start, time);
    {
        // The reference preintegrates here, in reserveNode (IMUManager::getFactor, GraphManager.cpp:59-66); so does this: K0 of the
        // new factor is enqueued on the engine's stream now, asynchronously (vf_engine_set_async), and the solve finds the
        // record in place instead of starting with a 60 us kernel.  Only when the slot exists already (no growth / compaction
        // pending) and every factor queued in front of it is on the device too (slots are consecutive); _stateMutex orders this
        // against a solve in flight, as getBias() above does.
        std::lock_guard<std::mutex> sl(g->state_mutex);
        const long slot = (long)(p.key - g->key_base);
        bool prev_ok = true;
        for (const auto& q : g->imu_queue) prev_ok = prev_ok && q.staged;
        if (prev_ok && !g->opts.synchronous_staging && slot >= 1 && slot < g->opts.capacity && p.key > g->key_base) {
            const int32_t off[2] = {0, (int32_t)(p.steps.size() / 7)};
            if (vf_engine_preintegrate(g->eng, 0, (int)slot, 1, off, p.steps.data(), p.bias, &g->imu) == VF_OK) p.staged = true;
        }
    }
    g->current_key++;
    g->imu_queue.push_back(std::move(p));
    g->last_pose_time = time;
    g->key_time.push_back(time);
    *key_out = g->current_key;
    return VF_OK;
}

int vf_add_imu_factor(vf_graph* g, uint64_t key, const double* rec190) {
    if (!g || !rec190) return gerr(VF_ERR_INVALID, "null argument");
    if (!(rec190[0] > 0.0) || !std::isfinite(rec190[0])) return gerr(VF_ERR_INVALID, "imu factor with deltaTij = %g", rec190[0]);
    for (int i = 0; i < VF_IMU_RECORD; i++)
        if (!std::isfinite(rec190[i])) return gerr(VF_ERR_INVALID, "imu factor record entry %d is not finite", i);
    for (int r = 0, o = 70; r < 15; o += 15 - r, r++)          // diagonal of the packed upper-triangular square-root information
        if (!(rec190[o] > 0.0)) return gerr(VF_ERR_NOT_SPD, "imu factor: square-root information has a non-positive diagonal entry (row %d)", r);
    std::lock_guard<std::mutex> lk(g->graph_mutex);  // GraphManager.cpp:92
    if (key != g->current_key + 1)
        return gerr(VF_ERR_BAD_KEY, "imu factor must end at the next key %llu (got %llu): keys are consecutive", (unsigned long long)(g->current_key + 1), (unsigned long long)key);
    if (g->opts.lag == 0 && g->opts.fixed_capacity && (int)(g->current_key + 1) >= g->opts.capacity) return gerr(VF_ERR_CAPACITY, "keyframe capacity %d exhausted", g->opts.capacity);
    PendingImu p;
    p.key = key;
    memset(p.bias, 0, sizeof(p.bias));
    p.record.assign(rec190, rec190 + VF_IMU_RECORD);
    g->current_key++;
    g->imu_queue.push_back(std::move(p));
    g->last_pose_time = (g->last_pose_time < 0.0 ? 0.0 : g->last_pose_time) + rec190[0];
    g->key_time.push_back(g->last_pose_time);
    return VF_OK;
}

int vf_get_most_recent_estimate(vf_graph* g, double q[4], double t[3], double v[3]) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);  // GraphManager.cpp:79
    // The reference never assigns _mostRecentEstimate (GraphManager.h:109; no write in GraphManager.cpp): the member
    // stays the default NavState -- identity pose, zero velocity -- for the life of the node.  Mirrored as it is.
    if (q) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }
    if (t) t[0] = t[1] = t[2] = 0.0;
    if (v) v[0] = v[1] = v[2] = 0.0;
    return VF_OK;
}

int vf_most_recent_pose_time(vf_graph* g, double* time, uint64_t* key) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (time) *time = g->last_pose_time;
    if (key) *key = g->current_key;
    return VF_OK;
}

// the 28-double record of a between factor from what the caller hands in, validated: vf_add_between and vf_gate_between
// (vf_graph_gate.cpp) refuse the same inputs with the same codes
int vf_between_record_(const double q[4], const double t[3], const double cov[36], double rec[VF_BTW_RECORD]) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.0) || !std::isfinite(n)) return gerr(VF_ERR_INVALID, "between rotation is not a quaternion");
    for (int i = 0; i < 4; i++) rec[i] = q[i] / n;  // gtsam::Rot3(w,x,y,z) normalises
    for (int i = 0; i < 3; i++) rec[4 + i] = t[i];
    if (!sqrt_info_upper6(cov, rec + 7)) return gerr(VF_ERR_NOT_SPD, "between covariance is not symmetric positive definite");
    return VF_OK;
}

int vf_add_between(vf_graph* g, uint64_t prev, uint64_t cur, const double q[4], const double t[3], const double cov[36]) {
    return vf_add_between_(g, prev, cur, q, t, cov, VF_LOSS_NONE, 0.0, nullptr);
}
// ... with a robust loss (vf_add_between_robust, vf_graph_robust.cpp, which has checked loss and loss_k)
int vf_add_between_(vf_graph* g, uint64_t prev, uint64_t cur, const double q[4], const double t[3], const double cov[36], int loss, double loss_k,
                    const vf_robust_calls* calls) {
    if (!g || !q || !t || !cov) return gerr(VF_ERR_INVALID, "null argument");
    PendingBetween b;
    b.a = prev;
    b.b = cur;
    b.loss = loss;
    b.loss_k = loss == VF_LOSS_NONE ? 0.0 : loss_k;
    if (int rc = vf_between_record_(q, t, cov, b.rec)) return rc;
    std::lock_guard<std::mutex> lk(g->graph_mutex);  // GraphManager.cpp:85
    if (prev >= cur || cur > g->current_key) return gerr(VF_ERR_BAD_KEY, "between factor keys (%llu, %llu) not reserved in order", (unsigned long long)prev, (unsigned long long)cur);
    bool band = cur - prev <= VF_MAX_BANDWIDTH && !g->has_band_end(cur);
    for (const auto& s : g->staged_between)
        if (s.b == cur) band = false;
    if (!band && loss != VF_LOSS_NONE && !g->robust_far)
        return gerr(VF_ERR_INVALID, "between factor (%llu, %llu) spans %llu keyframes or shares its end key: it would be a far factor, and far factors take no robust loss "
                    "on this handle (vf_set_robust_far is off)",(unsigned long long)prev, (unsigned long long)cur, (unsigned long long)(cur - prev));
    if (calls) { g->set_between_loss = calls->set_between_loss; g->set_far_robust = calls->set_far_robust; g->get_far_loss = calls->get_far_loss; }
    if (band) {
        g->staged_between.push_back(b);
    } else {
        // not a band factor: a far factor, solved as a low-rank correction (slower; include/vilfusion.h).  The list is bounded.
        if ((int)g->far_between.size() + g->far_linear.load() >= g->opts.max_far_factors)
            return gerr(VF_ERR_CAPACITY, "between factor (%llu, %llu) spans %llu keyframes or shares its end key, and the window already holds %d such factors "
                        "(vf_graph_opts.max_far_factors; at most %d)", (unsigned long long)prev, (unsigned long long)cur, (unsigned long long)(cur - prev),
                        g->opts.max_far_factors, VF_MAX_FAR_LIMIT);
        g->far_between.push_back(b);
        g->far_new++;
    }
    g->staged_count++;
    StagedFactor sf;
    sf.a = prev;
    sf.b = cur;
    memcpy(sf.q, b.rec, sizeof(sf.q));
    memcpy(sf.t, t, sizeof(sf.t));
    memcpy(sf.cov, cov, sizeof(sf.cov));
    sf.loss = b.loss;
    sf.loss_k = b.loss_k;
    g->staged_log.push_back(sf);
    return VF_OK;
}

// An absolute factor on `key` (vf_add_absolute_pose / vf_add_absolute_position, vf_graph_absolute.cpp): staged like a band factor from
// key - 1 -- it takes key's band slot, marks band_end at the take, and a later vf_add_between ending at key goes to the far list by
// the rule above.  A fix for a key already solved is written at the next solve, as late band odometry is; one whose key - 1 has left
// the window by then is dropped as late (refuse_late).
int vf_add_absolute_(vf_graph* g, uint64_t key, int kind, const double rec[VF_BTW_RECORD], const StagedFactor* shown, int loss, double loss_k,
                     vf_absolute_setter setter, const vf_robust_calls* calls) {
    if (!g || !rec || !shown || !setter) return gerr(VF_ERR_INVALID, "null argument");
    PendingBetween b;
    b.a = key - 1;
    b.b = key;
    b.kind = kind;
    b.loss = loss;
    b.loss_k = loss == VF_LOSS_NONE ? 0.0 : loss_k;
    memcpy(b.rec, rec, sizeof(b.rec));
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (key == 0 || key > g->current_key) return gerr(VF_ERR_BAD_KEY, "absolute factor on key %llu: not a reserved key other than the first", (unsigned long long)key);
    if (key - 1 < oldest_key(g))
        return gerr(VF_ERR_BAD_KEY, "absolute factor on key %llu: key %llu has left the window (oldest key %llu); the oldest keyframe cannot take one",
                    (unsigned long long)key, (unsigned long long)(key - 1), (unsigned long long)oldest_key(g));
    bool taken = g->has_band_end(key);
    for (const auto& s : g->staged_between) taken = taken || s.b == key;
    if (taken) return gerr(VF_ERR_CAPACITY, "absolute factor on key %llu: the key's band slot holds a factor already (one factor per slot)", (unsigned long long)key);
    g->set_absolute = setter;
    if (calls) { g->set_between_loss = calls->set_between_loss; g->set_far_robust = calls->set_far_robust; g->get_far_loss = calls->get_far_loss; }
    g->staged_between.push_back(b);
    g->staged_count++;
    StagedFactor sf = *shown;
    sf.a = key - 1;             // (as drop_late finds it; vf_graph_get_staged shows the key twice)
    sf.b = key;
    sf.kind = kind;
    sf.loss = b.loss;
    sf.loss_k = b.loss_k;
    g->staged_log.push_back(sf);
    return VF_OK;
}

int vf_set_callback(vf_graph* g, vf_callback cb, void* user) {
    if (!g || !cb) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    g->callbacks.emplace_back(cb, user);
    return VF_OK;
}

int vf_graph_staged(vf_graph* g, int* staged, int* queued) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (staged) *staged = g->staged_count;
    if (queued) *queued = (int)g->imu_queue.size();
    return VF_OK;
}

// GraphManager::graph() (GraphManager.cpp:46-49): the factors staged since the last solve, by index -- at first the three priors
// of :27-35 (kinds 0, 1, 2 on key 0), then the between factors in the order they were added (kind 3).
int vf_graph_get_staged(vf_graph* g, int index, int* kind, uint64_t* key1, uint64_t* key2, double q[4], double t[3], double cov36[36]) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    const int np = g->priors_staged ? 3 : 0;
    if (index < 0 || index >= np + (int)g->staged_log.size()) return gerr(VF_ERR_BAD_KEY, "staged factor %d of %d", index, np + (int)g->staged_log.size());
    if (q) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }
    if (t) t[0] = t[1] = t[2] = 0.0;
    if (cov36) memset(cov36, 0, sizeof(double) * 36);
    if (index < np) {
        // the means are the anchor state (identity / zero, or vf_set_initial_state's); sigmas vf_graph_opts.prior_sigma
        std::lock_guard<std::mutex> sl(g->state_mutex);
        const double* s = g->opts.prior_sigma;
        if (kind) *kind = index;
        if (key1) *key1 = 0;
        if (key2) *key2 = 0;
        if (index == 0) {
            if (q) memcpy(q, g->anchor, sizeof(double) * 4);
            if (t) memcpy(t, g->anchor + 4, sizeof(double) * 3);
            if (cov36) for (int i = 0; i < 6; i++) cov36[i * 6 + i] = s[i] * s[i];
        } else if (index == 1) {
            if (t) memcpy(t, g->anchor + 7, sizeof(double) * 3);
            if (cov36) for (int i = 0; i < 3; i++) cov36[i * 6 + i] = s[6 + i] * s[6 + i];
        } else {
            // (a bias has six components: acc in t, gyro in q[1..3]; documented in vilfusion.h)
            if (t) memcpy(t, g->anchor + 10, sizeof(double) * 3);
            if (q) { q[0] = 0.0; memcpy(q + 1, g->anchor + 13, sizeof(double) * 3); }
            if (cov36) for (int i = 0; i < 6; i++) cov36[i * 6 + i] = s[9 + i] * s[9 + i];
        }
        return VF_OK;
    }
    const StagedFactor& f = g->staged_log[(size_t)(index - np)];
    if (kind) *kind = 3 + f.kind;          // (3: a between factor; 4, 5: an absolute pose / position factor, on one key)
    if (key1) *key1 = f.kind == VF_ABSOLUTE_NONE ? f.a : f.b;
    if (key2) *key2 = f.b;
    if (q) memcpy(q, f.q, sizeof(f.q));
    if (t) memcpy(t, f.t, sizeof(f.t));
    if (cov36) memcpy(cov36, f.cov, sizeof(f.cov));
    return VF_OK;
}

// a far factor the engine can take: both keys inside the window
static bool in_window(const vf_graph* g, const PendingBetween& f, uint64_t last_key) { return f.a >= oldest_key(g) && f.b <= last_key; }
// the covariance of a solved key; the caller holds state_mutex
static int marginal_covariance(vf_graph* g, uint64_t key, double* cov225) {
    if (!g->solved_once) return gerr(VF_ERR_INVALID, "no solve yet: there is no covariance to report");
    if (key > g->solved_key) return gerr(VF_ERR_BAD_KEY, "key %llu not solved yet (last solved key %llu)", (unsigned long long)key, (unsigned long long)g->solved_key);
    if (key < oldest_key(g)) return gerr(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)key, (unsigned long long)oldest_key(g));
    if (!g->cov_valid || g->cov_tail) {      // (tail-only covariances, left by vf_gate_between, answer for the last two keys only: the full ones are computed)
        // (far_covariance: far factors alive, loop closures and what the marginalisation has left of them, downdate the band's
        // covariances; without it they are refused as they always were)
        g->cov_valid = g->cov_tail = false;
        if (int rc = g->opts.far_covariance ? vf_engine_marginals_ex(g->eng, VF_MARGINALS_FAR) : vf_engine_marginals(g->eng)) return rc;
        g->cov_valid = true;
        g->cov_pose = false;
    }
    return vf_engine_read_marginals(g->eng, 0, slot_of(g, key), 1, cov225, nullptr);
}
// Late odometry: a between factor whose older key is below the window's oldest key can never be added.  It is dropped -- from its
// list, from the staged log it is in (graph()'s list), from the counts --, the caller is told once, the rest is given back.
static bool is_late(const PendingBetween& f, uint64_t oldest) { return f.a < oldest; }
static void drop_late(std::vector<PendingBetween>& list, size_t i, std::vector<StagedFactor>& log, int& staged, int* far_new, LateFactor& first) {
    if (!first.any) first = {true, list[i].a, list[i].b};
    for (size_t j = 0; j < log.size(); j++)
        if (log[j].a == list[i].a && log[j].b == list[i].b) { log.erase(log.begin() + (long)j); break; }
    list.erase(list.begin() + (long)i);
    staged--;
    if (far_new) --*far_new;
}
static int late_error(const LateFactor& f, const char* when, uint64_t oldest) {
    return gerr(VF_ERR_BAD_KEY, "between factor (%llu, %llu) dropped: key %llu left the fixed-lag window%s (oldest key %llu)", (unsigned long long)f.a,
                (unsigned long long)f.b, (unsigned long long)f.a, when, (unsigned long long)oldest);
}
// take / give_back / publish_far_list: lock order is graph -> state everywhere (vf_reserve_node, vf_set_initial_state;
// GraphManager.cpp:54,60 -> 176), and the reference's solve() has released _graphMutex before it takes _stateMutex (:104-117): the
// three take graph_mutex themselves, before / after the state lock, never while it is held.  A solve that fails before the
// optimisation has run must not lose what it took from the queues: every step up to vf_engine_iterate is idempotent on the
// device (the same records, predictions and ranges are written again), so the take goes back to the FRONT of the queues and the
// next vf_solve repeats it.  solve_mutex (taken first, by vf_solve only) keeps a second solver from taking newer entries between
// the failure and the give-back.
// under _graphMutex: emptyImuQueue + snapshot of the staged factors (GraphManager.cpp:104-114)
static void take(vf_graph* g, SolveTake& t) {
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    t.imus.swap(g->imu_queue);
    t.betweens.swap(g->staged_between);
    t.set_loss = g->set_between_loss;
    t.set_far_robust = g->set_far_robust;
    t.get_far_loss = g->get_far_loss;
    t.set_absolute = g->set_absolute;
    for (const auto& bt : t.betweens) g->set_band_end(bt.b, 1);   // these keys now carry their band factor (a second one goes to the far list)
    // (keys below the window can never be named again by a factor that is accepted: their marks are let go)
    while (!g->band_end.empty() && g->band_base < oldest_key(g)) { g->band_end.pop_front(); g->band_base++; }
    // A far factor whose older key has left the window (as of the previous solve: lo / key_base change under solve_mutex,
    // which this thread holds) is no business of this list: one that was on the device then was marginalised with its key and
    // lives on in the engine (the list was replaced after that solve's marginalisations); one that was added SINCE that solve
    // never made it into the window.  Late odometry: the new ones only, all at once, reported by the first (refuse_late)
    const uint64_t oldest = oldest_key(g);
    auto& fb = g->far_between;
    for (size_t i = fb.size() - (size_t)g->far_new; i < fb.size();)
        if (is_late(fb[i], oldest)) drop_late(fb, i, g->staged_log, g->staged_count, &g->far_new, t.late_far);
        else i++;
    fb.erase(std::remove_if(fb.begin(), fb.end(), [oldest](const PendingBetween& f) { return is_late(f, oldest); }), fb.end());
    t.fars = fb;
    t.fars_snapshot = fb.size();
    std::swap(t.far_new, g->far_new);
    std::swap(t.staged, g->staged_count);  // _graph->resize(0)
    t.log.swap(g->staged_log);
    std::swap(t.priors, g->priors_staged);
    t.last_key = g->current_key, t.last_time = g->last_pose_time;
}
static void give_back(vf_graph* g, SolveTake& t) {
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    for (auto it = t.imus.rbegin(); it != t.imus.rend(); ++it) g->imu_queue.push_front(std::move(*it));
    g->staged_between.insert(g->staged_between.begin(), t.betweens.begin(), t.betweens.end());
    g->staged_count += t.staged;
    g->staged_log.insert(g->staged_log.begin(), t.log.begin(), t.log.end());
    g->priors_staged = g->priors_staged || t.priors;
    // the far factors added since the last successful solve are still "new" for the solve that repeats this one (its
    // late-odometry test looks at the new ones only), and a band factor dropped as late leaves its end key free again
    g->far_new += t.far_new;
    if (t.late_band.any) g->set_band_end(t.late_band.b, 0);
}
// the entries taken are the front of the list (others only append, under graph_mutex): replace them by their current form
// (the ones the engine has taken over are gone; on_device marks)
static void publish_far_list(vf_graph* g, SolveTake& t) {
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (g->far_between.size() < t.fars_snapshot) return;
    std::vector<PendingBetween> now(t.fars);
    now.insert(now.end(), g->far_between.begin() + (long)t.fars_snapshot, g->far_between.end());
    g->far_between.swap(now);
}
// The steps of a solve, in the order vf_solve runs them, under state_mutex.  Host-side validation first: late odometry
static int refuse_late(vf_graph* g, SolveTake& t) {
    const uint64_t oldest = oldest_key(g);
    if (t.late_far.any) return late_error(t.late_far, "", oldest);
    // band factors: the first late one only per solve; its end key carries no band factor after all (give_back clears the mark)
    for (size_t i = 0; i < t.betweens.size(); i++)
        if (is_late(t.betweens[i], oldest)) {
            drop_late(t.betweens, i, t.log, t.staged, nullptr, t.late_band);
            return late_error(t.late_band, "", oldest);
        }
    return VF_OK;
}
static int make_room(vf_graph* g, SolveTake& t, Lap& lap) {
    if (slot_of(g, t.last_key) + 1 <= g->opts.capacity) return VF_OK;
    if (g->opts.lag == 0) {
        // whole-history mode (the reference's unbounded graph): the engine grows with the history
        int want = g->opts.capacity;
        while (slot_of(g, t.last_key) + 1 > want) want *= 2;
        if (int rc = vf_engine_grow(g->eng, want)) return rc;
        g->opts.capacity = want;
        lap("grow");
        return VF_OK;
    }
    // fixed-lag mode: reclaim slots below the window when the new keyframes would not fit
    const int shift = (g->lo / 64) * 64;
    if (shift <= 0) return gerr(VF_ERR_CAPACITY, "capacity %d too small for lag %d plus the keyframes added per solve", g->opts.capacity, g->opts.lag);
    if (int rc = vf_engine_compact(g->eng, shift)) return rc;
    g->lo -= shift, g->key_base += shift;
    if (slot_of(g, t.last_key) + 1 > g->opts.capacity) return gerr(VF_ERR_CAPACITY, "capacity %d exhausted even after compaction", g->opts.capacity);
    return VF_OK;
}
// fixed-lag window: marginalise the keyframes that fall out of the lag, one at a time, at the linearisation of the previous
// solve (their factors have not changed since).  FIRST: the engine runs it on a second stream, beside the preintegration /
// prediction / staging of the keyframes that arrive (vf_engine_set_async)
static int marginalise(vf_graph* g, SolveTake& t, Lap& lap) {
    while (g->opts.lag > 0 && slot_of(g, t.last_key) + 1 - g->lo > g->opts.lag && slot_of(g, g->solved_key) - g->lo >= 3) {
        if (int rc = vf_engine_marginalize(g->eng)) return rc;
        if (int rc = vf_engine_drop_oldest(g->eng)) return rc;
        g->lo++;      // (kept in step with the device: a keyframe that has been marginalised stays marginalised)
        t.marginalised = true;
    }
    lap("marginalize");
    // Late odometry: far factors whose older key the loop has just moved out of the window and that never reached the device
    // (the engine has marginalised the others with their key), all at once, reported by the first, "in this solve".  (A band
    // factor in that position has passed refuse_late and is staged below the window, where the kernels ignore it: ADVICE.md.
    // Refusing it is one more drop_late here, over t.betweens with refuse_late's marks; that call is deliberately not made yet.)
    const uint64_t oldest = oldest_key(g);
    LateFactor late;
    for (size_t i = 0; i < t.fars.size();)
        if (!t.fars[i].on_device && is_late(t.fars[i], oldest)) drop_late(t.fars, i, t.log, t.staged, &t.far_new, late);
        else i++;
    t.fars_changed = t.fars_changed || late.any;
    return late.any ? late_error(late, " in this solve", oldest) : VF_OK;
}
// K0 on the device for all queued factors, then the initial values by IMU prediction (GraphManager.cpp:150-160); keys are consecutive
static int stage_imu(vf_graph* g, SolveTake& t, Lap& lap) {
    if (t.imus.empty()) return VF_OK;
    const auto& imus = t.imus;
    const int n = (int)imus.size(), k0 = slot_of(g, imus.front().key);
    // runs of factors cut from the IMU buffer (reserveNode) are preintegrated in one K0 launch; ready-made factors (addFactor) are staged as records
    for (int i = 0; i < n;) {
        int j = i;
        if (imus[i].staged) { i++; continue; }          // preintegrated at reserveNode time: the record is on the device
        const bool ready = !imus[i].record.empty();
        while (j < n && !imus[j].staged && imus[j].record.empty() == !ready) j++;
        const int cnt = j - i;
        if (ready) {
            std::vector<double> recs((size_t)cnt * VF_IMU_RECORD);
            for (int l = 0; l < cnt; l++) memcpy(&recs[(size_t)l * VF_IMU_RECORD], imus[i + l].record.data(), sizeof(double) * VF_IMU_RECORD);
            if (int rc = vf_engine_set_imu(g->eng, 0, k0 + i, cnt, recs.data())) return rc;
        } else {
            std::vector<int32_t> off(cnt + 1, 0);
            std::vector<double> steps, bias((size_t)cnt * 6);
            for (int l = 0; l < cnt; l++) {
                off[l + 1] = off[l] + (int)(imus[i + l].steps.size() / 7);
                steps.insert(steps.end(), imus[i + l].steps.begin(), imus[i + l].steps.end());
                memcpy(&bias[(size_t)l * 6], imus[i + l].bias, sizeof(double) * 6);
            }
            if (int rc = vf_engine_preintegrate(g->eng, 0, k0 + i, cnt, off.data(), steps.data(), bias.data(), &g->imu)) return rc;
        }
        i = j;
    }
    lap("preintegrate");
    // reference_compat: from the ESTIMATE of the last keyframe (_currentState, GraphManager.cpp:152), not its linearisation point
    if (int rc = (g->opts.reference_compat && g->solved_key > 0) ? vf_engine_predict_from_estimate(g->eng, 0, k0, n) : vf_engine_predict(g->eng, 0, k0, n)) return rc;
    lap("predict");
    return VF_OK;
}
static int stage_band(vf_graph* g, SolveTake& t, Lap& lap) {
    const auto& betweens = t.betweens;
    if (betweens.empty()) return VF_OK;
    std::vector<int32_t> a(betweens.size()), b(betweens.size());
    std::vector<double> rec(betweens.size() * VF_BTW_RECORD);
    // the engine wants runs sorted by b
    std::vector<size_t> order(betweens.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    for (size_t i = 1; i < order.size(); i++)
        for (size_t j = i; j > 0 && betweens[order[j]].b < betweens[order[j - 1]].b; j--) std::swap(order[j], order[j - 1]);
    for (size_t i = 0; i < order.size(); i++) {
        a[i] = slot_of(g, betweens[order[i]].a);
        b[i] = slot_of(g, betweens[order[i]].b);
        memcpy(&rec[i * VF_BTW_RECORD], betweens[order[i]].rec, sizeof(double) * VF_BTW_RECORD);
    }
    // (absolute factors among them go through their own call, the others through vf_engine_set_between: two sorted subsequences)
    std::vector<int32_t> ua, ub, uk;
    std::vector<double> urec;
    bool unary = false;
    for (const auto& f : betweens) unary = unary || f.kind != VF_ABSOLUTE_NONE;
    if (!unary) {
        if (int rc = vf_engine_set_between(g->eng, 0, (int)a.size(), a.data(), b.data(), rec.data())) return rc;
    } else {
        if (!t.set_absolute) return gerr(VF_ERR_INVALID, "an absolute factor is staged and the handle has no call to send it with");
        std::vector<int32_t> pa, pb;
        std::vector<double> prec;
        for (size_t i = 0; i < order.size(); i++) {
            const PendingBetween& f = betweens[order[i]];
            const double* r = &rec[i * VF_BTW_RECORD];
            if (f.kind == VF_ABSOLUTE_NONE) { pa.push_back(a[i]); pb.push_back(b[i]); prec.insert(prec.end(), r, r + VF_BTW_RECORD); }
            else { ub.push_back(b[i]); uk.push_back(f.kind); urec.insert(urec.end(), r, r + VF_BTW_RECORD); }
        }
        if (!pa.empty())
            if (int rc = vf_engine_set_between(g->eng, 0, (int)pa.size(), pa.data(), pb.data(), prec.data())) return rc;
        if (int rc = t.set_absolute(g->eng, 0, (int)ub.size(), ub.data(), uk.data(), urec.data())) return rc;
    }
    lap("set_between");
    // the losses behind the records (the engine resets the slots it writes): only when one of these factors has a loss
    bool robust = false;
    for (const auto& f : betweens) robust = robust || f.loss != VF_LOSS_NONE;
    if (robust && t.set_loss) {
        std::vector<int32_t> loss(betweens.size());
        std::vector<double> k(betweens.size());
        for (size_t i = 0; i < order.size(); i++) { loss[i] = betweens[order[i]].loss; k[i] = betweens[order[i]].loss_k; }
        if (int rc = t.set_loss(g->eng, 0, (int)b.size(), b.data(), loss.data(), k.data())) return rc;
        lap("set_between_loss");
    }
    return VF_OK;
}
// the engine has marginalised the far factors whose older key left together with that key (they are linear rows of its own now):
// the entries that were on the device are replaced by what the engine's list holds now
static int adopt_engine_far_list(vf_graph* g, SolveTake& t) {
    if (!t.marginalised || !(g->far_on_device || g->far_linear.load() > 0)) return VF_OK;
    int rc, cnt = 0, lin = 0;
    int32_t ea[VF_MAX_FAR_LIMIT], eb[VF_MAX_FAR_LIMIT];
    double erec[VF_MAX_FAR_LIMIT * VF_BTW_RECORD];
    if ((rc = vf_engine_get_extra_between(g->eng, 0, &cnt, ea, eb, erec, nullptr, nullptr, nullptr))) return rc;
    // ... and the loss of every entry with it (an attribute of the list entry: the engine's list has kept each on its own through the
    // marginalisation).  A handle that was never given a robust factor has no call to make and no loss to lose
    int32_t eloss[VF_MAX_FAR_LIMIT] = {0};
    double ek[VF_MAX_FAR_LIMIT] = {0};
    if (t.get_far_loss && (rc = t.get_far_loss(g->eng, 0, eloss, ek))) return rc;
    std::vector<PendingBetween> moved;
    for (int i = 0; i < cnt; i++) {
        PendingBetween f;
        f.a = (uint64_t)ea[i] + g->key_base, f.b = (uint64_t)eb[i] + g->key_base;
        memcpy(f.rec, erec + (size_t)i * VF_BTW_RECORD, sizeof(f.rec));
        f.on_device = true;
        f.loss = eloss[i], f.loss_k = ek[i];
        moved.push_back(f);
    }
    for (const auto& f : t.fars)
        if (!f.on_device) moved.push_back(f);
    t.fars.swap(moved);
    t.fars_changed = true;
    if ((rc = vf_engine_get_linear_far(g->eng, 0, &lin, nullptr))) return rc;
    g->far_linear.store(lin);
    return VF_OK;
}
// far between factors still inside the window, in window-local slots (the engine ignores one whose older keyframe is below
// `lo`; the list is re-sent at every solve, so compaction and growth need no bookkeeping here)
static int stage_far_list(vf_graph* g, SolveTake& t, Lap& lap) {
    if (t.fars.empty() && !g->far_on_device) return VF_OK;
    std::vector<int32_t> a, b, loss;
    std::vector<double> rec, k;
    bool robust = false;
    for (const auto& f : t.fars) {
        if (!in_window(g, f, t.last_key)) continue;
        a.push_back(slot_of(g, f.a));
        b.push_back(slot_of(g, f.b));
        rec.insert(rec.end(), f.rec, f.rec + VF_BTW_RECORD);
        loss.push_back(f.loss);
        k.push_back(f.loss_k);
        robust = robust || f.loss != VF_LOSS_NONE;
    }
    // (the losses travel with the list; a list without one is the plain call, which also clears what an earlier list carried)
    if (robust && !t.set_far_robust) return gerr(VF_ERR_INVALID, "a far factor carries a loss and the handle has no call to send it with");
    if (int rc = robust ? t.set_far_robust(g->eng, 0, (int)a.size(), a.data(), b.data(), rec.data(), loss.data(), k.data())
                        : vf_engine_set_extra_between(g->eng, 0, (int)a.size(), a.data(), b.data(), rec.data())) return rc;
    g->far_on_device = !a.empty();
    for (auto& f : t.fars)
        if (in_window(g, f, t.last_key)) { t.fars_changed = t.fars_changed || !f.on_device; f.on_device = true; }
    lap("set_extra");
    return VF_OK;
}
static int optimise_and_read(vf_graph* g, SolveTake& t, Lap& lap, int& fails, int& flags) {
    const int last_slot = slot_of(g, t.last_key);
    lap("set_range");
    if (g->opts.reference_compat) {
        if (int rc = vf_engine_isam_step(g->eng, g->opts.relin_threshold)) return rc;  // one ISAM2::update
        lap("isam_step");
        if (int rc = vf_engine_read_result(g->eng, 0, last_slot, 1, g->state, nullptr, nullptr, nullptr, nullptr, &flags)) return rc;   // calculateEstimate, :127,131-133
    } else {
        if (int rc = vf_engine_iterate(g->eng, g->opts.iterations)) return rc;   // (ISAM2::update + calculateEstimate: LM to convergence)
        lap("iterate(launch)");
        // the one synchronisation of the solve: the last state (:131-133), the failure count, what the staging kernels flagged
        if (int rc = vf_engine_read_result(g->eng, 0, last_slot, 0, g->state, nullptr, nullptr, nullptr, &fails, &flags)) return rc;
    }
    lap("read_result(sync)");
    return VF_OK;
}
static int publish(vf_graph* g, SolveTake& t, int fails, int flags) {
    // (asynchronous staging: a preintegrated covariance / a marginalisation pivot that was not positive definite shows here, after
    // the solve that used it -- with positive IMU covariances and a determined graph neither happens)
    if (flags & 1) return gerr(VF_ERR_NOT_SPD, "preintegrated covariance not positive definite");
    if (flags & 6) return gerr(VF_ERR_INDETERMINATE, "marginalisation: %s not positive definite", (flags & 4) ? "the far ends' block of the marginal" : "pivot block of the oldest keyframe");
    g->solved_key = t.last_key;
    g->solved_once = true;
    // covariance callbacks (no reference code): the marginal covariance of the solved keyframe, computed only while one is registered
    double cov[225];
    if (!g->cov_callbacks.empty() && marginal_covariance(g, t.last_key, cov) != VF_OK)
        for (double& c : cov) c = std::numeric_limits<double>::quiet_NaN();
    for (auto& cb : g->callbacks)  // :135-138, on the solving thread, inside _stateMutex
        cb.first(cb.second, t.last_time, g->state, g->state + 4, g->state + 7, g->state + 10);
    for (auto& cb : g->cov_callbacks)
        cb.first(cb.second, t.last_time, g->state, g->state + 4, g->state + 7, g->state + 10, cov);
    // a full fixed-lag window marginalises its oldest keyframe at the next update, from the linearisation this solve leaves:
    // have the device compute that marginal prior now, behind the solve, instead of in front of the next one
    if (g->opts.lag > 0 && !g->opts.synchronous_staging && slot_of(g, t.last_key) + 1 - g->lo >= g->opts.lag) (void)vf_engine_marginalize_ahead(g->eng);
    if (fails > 0 && fails >= g->opts.iterations && g->opts.iterations > 0)
        return gerr(VF_ERR_INDETERMINATE, "normal equations not positive definite in every LM trial (underdetermined graph?)");
    return VF_OK;
}

int vf_solve(vf_graph* g) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    Lap lap;
    SolveTake t;
    std::lock_guard<std::mutex> solve_lk(g->solve_mutex);
    take(g, t);
    int rc, fails = 0, flags = 0;
    {
        std::lock_guard<std::mutex> sl(g->state_mutex);  // :117
        g->cov_valid = g->cov_tail = g->err_valid = false;
        (rc = refuse_late(g, t)) || (rc = make_room(g, t, lap)) || (rc = marginalise(g, t, lap)) || (rc = stage_imu(g, t, lap)) || (rc = stage_band(g, t, lap)) ||
            (rc = adopt_engine_far_list(g, t)) || (rc = stage_far_list(g, t, lap)) || (rc = vf_engine_set_range(g->eng, 0, g->lo, slot_of(g, t.last_key) + 1));
        t.requeue = rc != VF_OK;    // up to here a failure gives the take back; the optimisation consumes it, whatever it returns
        if (!rc) rc = optimise_and_read(g, t, lap, fails, flags);
        if (!rc) rc = publish(g, t, fails, flags);
    }
    if (t.fars_changed) publish_far_list(g, t);
    if (t.requeue) give_back(g, t);
    return rc;
}

int vf_get_state(vf_graph* g, double q[4], double t[3], double v[3], double bias[6]) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (q) memcpy(q, g->state, sizeof(double) * 4);
    if (t) memcpy(t, g->state + 4, sizeof(double) * 3);
    if (v) memcpy(v, g->state + 7, sizeof(double) * 3);
    if (bias) memcpy(bias, g->state + 10, sizeof(double) * 6);
    return VF_OK;
}

int vf_get_marginal_covariance(vf_graph* g, uint64_t key, double cov225[225]) {
    if (!g || !cov225) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    return marginal_covariance(g, key, cov225);
}

int vf_set_covariance_callback(vf_graph* g, vf_cov_callback cb, void* user) {
    if (!g || !cb) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    g->cov_callbacks.emplace_back(cb, user);
    return VF_OK;
}

int vf_get_bias(vf_graph* g, double bias[6]) { return vf_get_state(g, nullptr, nullptr, nullptr, bias); }

int vf_graph_lm_stats(vf_graph* g, double* cost, int* accepted, int* rejected, int* solve_failures) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    return vf_engine_read_lm(g->eng, 0, cost, nullptr, accepted, rejected, solve_failures);
}

int vf_graph_solver_info(vf_graph* g, int* window_keyframes, int* refine_corrections, int* provisional_trials) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (window_keyframes) *window_keyframes = slot_of(g, g->solved_key) + 1 - g->lo;
    int rc;
    if (refine_corrections && (rc = vf_engine_refine_count(g->eng, refine_corrections))) return rc;
    if (provisional_trials && (rc = vf_engine_read_excursions(g->eng, 0, provisional_trials, nullptr))) return rc;
    return VF_OK;
}

int vf_graph_incremental_info(vf_graph* g, long* updates, long* whole_window_updates, uint64_t* first_eliminated_key, uint64_t* last_substituted_key) {
    if (!g) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    int a = -1, b = -1;
    if (int rc = vf_engine_incremental_info(g->eng, 0, updates, whole_window_updates, &a, &b)) return rc;
    if (first_eliminated_key) *first_eliminated_key = a < 0 ? 0 : (uint64_t)a + g->key_base;
    if (last_substituted_key) *last_substituted_key = b < 0 ? 0 : (uint64_t)b + g->key_base;
    return VF_OK;
}

int vf_get_trajectory(vf_graph* g, uint64_t key0, int n, double* state16) {
    if (!g || !state16) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (n < 0 || key0 + (uint64_t)n > g->solved_key + 1) return gerr(VF_ERR_BAD_KEY, "keys [%llu, %llu) not solved yet", (unsigned long long)key0, (unsigned long long)(key0 + n));
    if (key0 < g->key_base) return gerr(VF_ERR_BAD_KEY, "key %llu has been compacted away (oldest retained key %llu)", (unsigned long long)key0, (unsigned long long)g->key_base);
    if (g->opts.reference_compat) return vf_engine_get_estimate(g->eng, 0, slot_of(g, key0), n, state16);
    return vf_engine_get_states(g->eng, 0, slot_of(g, key0), n, state16);
}

int vf_get_imu_factor(vf_graph* g, uint64_t key, double* rec190) {
    if (!g || !rec190) return gerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (key < 1 || key > g->solved_key || key < g->key_base + 1) return gerr(VF_ERR_BAD_KEY, "imu factor %llu not on the device", (unsigned long long)key);
    return vf_engine_get_imu(g->eng, 0, slot_of(g, key), 1, rec190);
}

}  // extern "C"
