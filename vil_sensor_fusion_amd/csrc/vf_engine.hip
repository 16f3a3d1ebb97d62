// vf_engine.hip -- host side of the batch engine behind include/vilfusion.h.
// Owns the HBM-resident problem (vf::View), stages host AoS records into the AoSoA device
// layout, and sequences the hot-path kernels on one HIP stream.  There is no CPU fallback:
// without a gfx950 device every entry point fails with VF_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include <dlfcn.h>

#include "../../include/vilfusion.h"
#include "vf_kernels.hpp"
#include "vf_launch_view.hpp"
#include "vf_device_buf.hpp"
#include "vf_upload_channel.hpp"
#include "vf_engine_memory.hpp"

namespace {
thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(VF_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                  \
    } while (0)
vf::ImuCov imu_cov(const vf_imu_params* p) { return {p->acc_cov, p->gyro_cov, p->integration_cov, p->bias_acc_cov, p->bias_omega_cov, p->bias_acc_omega_int}; }
}  // namespace

struct vf_engine;
// The head of every entry point that takes an engine, in one line: the engine (null: nothing happens, the entry point refuses
// it next), whether the call may overlap the side stream's work (see EngineHandle::side_open), what it does to what the device
// holds from the last solve (vf_engine_memory.hpp), and whether it leaves the cached result block alone.  From these it joins
// the side stream, voids the cached result, fires the event, and makes the engine's device current for the duration of the
// call -- HIP's current device is per host thread: allocations, copies and launches would otherwise go to whatever device
// the calling thread last used (e.g. a ROS spinner thread driving a GraphManager on device 1) -- restoring the caller's on return.
struct Entry {
    struct Effect { int kind, window, slot; };
    static constexpr Effect reads{0, 0, 0}, rewrites{2, 0, 0};
    static constexpr Effect appends(int window, int slot) { return {1, window, slot}; }
    enum { overlaps = 1, leaves_result = 2 };
    static constexpr int overlaps_if(bool yes) { return yes ? overlaps : 0; }
    Entry(vf_engine* e, Effect does, int flags = 0);
    ~Entry() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
    Entry(const Entry&) = delete;
    Entry& operator=(const Entry&) = delete;
    vf_engine* const engine;
    int prev = -1, want = -1;
};
// ... and the refusal of a null engine with it
#define VF_ENTER(...) Entry entry_(__VA_ARGS__); if (!entry_.engine) return fail(VF_ERR_INVALID, "engine is null")

// What belongs to the HANDLE the caller holds: it stays when vf_engine_grow replaces the arrays behind it.
struct EngineHandle {
    hipStream_t stream = nullptr;
    bool own_stream = true;   // false once the caller has handed in its own stream (vf_engine_set_stream)
    // Asynchronous staging (vf_engine_set_async; the GraphManager's engine): the staging calls of a vf_solve -- preintegrate,
    // set_between, marginalize, drop_oldest, set_range -- enqueue and return; what the device finds wrong (a preintegrated
    // covariance or a marginalisation pivot that is not positive definite) is OR-ed into two sticky words that
    // vf_engine_read_result hands back with the solve's result, in the one synchronisation a solve needs.  The marginalisation
    // of the keyframe that leaves runs on a second stream beside K0 / prediction / staging of the one that arrives (they
    // touch opposite ends of the window): side_open until the main stream has been made to wait for it (join_side, at
    // every entry point that is not one of those three).
    bool async_on = false, side_open = false;
    hipStream_t stream2 = nullptr;
    vf::Event ev_fork, ev_join;
    vf::DeviceBuf<int> sticky_dev;
    vf::PinnedBuf<vf::SolveResult> res_host;
    long far_transported = 0, far_ended = 0, far_absorbed = 0;   // far factors moved on to the next keyframe when theirs left the window /
                                                                 // dropped without a marginalisation / absorbed into the marginal prior
    bool marg_since_drop = false;   // vf_engine_marginalize ran since the last vf_engine_drop_oldest (the GraphManager's call pair)
    long inc_updates = 0, inc_full = 0;      // incremental updates so far; those that eliminated from the window's first keyframe
};

// ... and everything else belongs to the device ARRAYS (and what the host knows about them), which a grown engine replaces whole
struct vf_engine : EngineHandle {
    vf::View v{};            // holds the neutral value of every per-launch word, always: launches that differ take a copy (vf_launch_view.hpp)
    vf::SolveMemory mem;     // what the arrays still hold from the last solve
    vf_engine_opts opts{};
    vf_engine_tuning tune{};
    // vf_engine_opts.use_hip_graph: vf_engine_iterate replays its launch sequence (6 + 9 K kernels / memsets) from a captured
    // hipGraph; re-captured when the trial count or any scalar baked into the kernel arguments changes
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_iters = -1, graph_mode = 0;
    long graph_epoch = -1, epoch = 0;
    bool graph_off = false;
    long graph_replays = 0;          // hipGraphLaunch calls so far; graph_captures: (re-)captures of the sequence
    int graph_captures = 0;
    double* lambda0_dev = nullptr;   // [B] lambda0, the source of the per-solve reset
    void drop_graph() {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        graph_exec = nullptr;
        graph = nullptr;
        graph_iters = -1;
    }
    vf::Event ev0, ev1;
    std::vector<void*> allocs;
    // What is made after creation -- on first use, or grown on demand -- owns itself (vf_device_buf.hpp): `delete` frees it, and
    // vf_engine_grow moves it with the arrays, or leaves it with the handle, like every other member
    vf::DeviceBuf<double> stage;  // device staging buffer (AoS)
    int ensure_stage(size_t bytes) { HIPCHK(stage.ensure(bytes)); return VF_OK; }
    double* sigma_dev = nullptr;
    double sigma_host[15] = {0};    // what sigma_dev holds (vf_engine_slide uploads only a changed set)
    bool sigma_valid = false;
    int* status_dev = nullptr;
    std::vector<int> h_lo, h_hi;  // host mirror of the active ranges
    // The adaptive trial loop of vf_engine_iterate reads the whole result block where it used to read the `done` flag: when the flag
    // is up the solve is over and the block IS the result -- the vf_engine_read_result that follows finds it in res_host
    // (SolveMemory::result_cached_for, until any other entry point runs) and costs no second synchronisation.
    int ensure_async() {          // the sticky words and the pinned result block (every engine may be asked for a vf_engine_read_result)
        if (res_host) return VF_OK;
        HIPCHK(sticky_dev.ensure(2 * sizeof(int)));
        HIPCHK(hipMemsetAsync(sticky_dev, 0, 2 * sizeof(int), stream));
        HIPCHK(res_host.ensure(sizeof(vf::SolveResult)));
        return VF_OK;
    }
    int ensure_side() {           // the second stream (hipStreamCreate costs 9 ms: only engines that stage asynchronously get one)
        if (stream2) return VF_OK;
        HIPCHK(hipStreamCreate(&stream2));
        HIPCHK(ev_fork.ensure(hipEventDisableTiming));
        HIPCHK(ev_join.ensure(hipEventDisableTiming));
        return VF_OK;
    }
    int join_side() {
        if (!side_open) return VF_OK;
        side_open = false;
        HIPCHK(hipEventRecord(ev_join, stream2));
        HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
        return VF_OK;
    }
    // async_base: staging calls enqueue and return.  async_now: ... and the window holds no far factors -- the marginalisation may run
    // on the second stream / ahead of time (k_marginalize<0> only; with far factors alive it reads and rewrites their lists, which
    // the host re-sends on the main stream).  async_far: the rest -- the marginalisation enqueued on the main stream.
    bool async_base() const { return async_on && v.B == 1 && own_stream; }
    bool async_now() const { return async_base() && x_used == 0; }
    bool async_far() const { return async_base() && x_used > 0; }
    // vf_engine_marginalize_ahead: the marginal prior the next vf_engine_marginalize will need, computed behind the solve that has
    // just ended (the linearisation it reads is final by then) into marg_stash (SolveMemory::stash_fits)
    vf::DeviceBuf<double> marg_stash;
    // hybrid K4 (vf_kernels.hpp "View::gate"): buffers and chunk count of the partitioned form for a sweep engine, allocated
    // when the termination rule is first switched on
    bool hybrid = false;
    int hybrid_P = 0;
    double *h_Vp = nullptr, *h_sep = nullptr, *h_sepL = nullptr;
    int* act_list = nullptr;   // compacted list of the windows still taking trials (vf_engine_opts.hybrid_active_list): handed to the hybrid's
                               // sweeps and to k_count_active only -- every other launch sees View::act = null
    vf::View partitioned_view() const { return vf::partitioned_form(v, hybrid_P, h_Vp, h_sep, h_sepL); }

    // The arrays of an engine are carved out of ONE device allocation made at creation (reserve(): a hipMalloc costs 0.1-0.3 ms
    // whatever its size, and an engine has forty arrays -- creating the 6-window column engine of a first loop closure inside a
    // vf_solve took 13 ms of which the memory itself was the least); what does not fit, or comes later, is allocated on its own.
    char* arena = nullptr;
    size_t arena_size = 0, arena_used = 0;
    int reserve(size_t bytes) {
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, bytes));
        allocs.push_back(q);
        HIPCHK(hipMemsetAsync(q, 0, bytes, stream));
        arena = (char*)q;
        arena_size = bytes;
        arena_used = 0;
        return VF_OK;
    }
    template <typename T>
    int alloc(T** p, size_t n, bool zero = true) {
        const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        if (arena && arena_used + bytes <= arena_size) {
            *p = (T*)(arena + arena_used);           // (zeroed by reserve())
            arena_used += bytes;
            return VF_OK;
        }
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, n * sizeof(T)));
        allocs.push_back(q);
        if (zero) HIPCHK(hipMemsetAsync(q, 0, n * sizeof(T), stream));
        *p = (T*)q;
        return VF_OK;
    }
    // grow-only scratch of vf_engine_preintegrate (the GraphManager calls it once per solve: no hipMalloc / hipFree there)
    vf::DeviceBuf<char> pre_buf;
    int ensure_pre(size_t bytes) {
        HIPCHK(pre_buf.ensure(bytes, [](size_t b) { return b < (1u << 16) ? (size_t)1 << 16 : b * 2; }));
        return VF_OK;
    }
    // The argument blocks of vf_engine_ingest_tail (and of an asynchronous vf_engine_preintegrate), vf_engine_propagate_tail and
    // vf_engine_gate_tail travel through a channel each (vf_upload_channel.hpp: pinned block, device twin, the events that time the
    // copy and the kernel): on asynchronous engines any of them may be in flight while another is used.  Made by the first call.
    vf::UploadChannel ingest, prop, gate;
    // ... and what the kernels write: the sticky status word of the ingest, the propagation's [B][16 + 225], the gate's [B] records of
    // vf_gate_result's layout.  Whether the last two hold anything is SolveMemory's to say (propagation_valid, gate_valid).
    vf::DeviceBuf<int> in_status;
    vf::DeviceBuf<double> prop_out;
    vf::DeviceBuf<char> gate_out;
    // vf_engine_gate_closures (engine/engine_closure.inc): its argument block's channel; what its kernels write (records, then the
    // joint covariances); the scratch of a group of windows (unit columns, and Z and C of the far systems); the zero lambda, failure
    // flags and all-ones `fresh` flags of its undamped factorisation (the marginals' own live in sig, which this call never makes).
    // All made by the first call: an engine that never gates closures holds none.  How many records there are to read is
    // SolveMemory's to say (closure_gate_count)
    vf::UploadChannel closure;
    vf::DeviceBuf<char> cg_out;
    vf::DeviceBuf<double> cg_scratch, cg_aux;
    double* cg_zero() const { return cg_aux; }
    int* cg_fail() const { return (int*)(cg_aux + v.B); }
    int* cg_ones() const { return cg_fail() + v.B; }
    int ensure_ingest() {
        if (in_status) return VF_OK;
        HIPCHK(in_status.ensure(sizeof(int)));
        HIPCHK(hipMemsetAsync(in_status, 0, sizeof(int), stream));
        return VF_OK;
    }
    // far between factors (View::x_*): host mirror of how many slots are in use (the low-rank correction solves 6 right-hand
    // sides per slot in use), the right-hand-side scratch and the solved columns Z
    int x_used = 0;
    std::vector<int> h_xn;
    std::vector<std::vector<int>> h_xa, h_xb;          // host copies of every window's list (re-sent after compact / grow)
    std::vector<char> h_xdirty;                        // the device's copy of a window's list may differ from the host's (k_marginalize has
                                                       // struck out entries the host has not yet): vf_engine_set_extra_between must re-send
    std::vector<std::vector<double>> h_xrec;
    // ... and the robust loss of every entry (vf_engine_set_extra_between_robust): an attribute of the list ENTRY, so it goes wherever the
    // list goes -- these mirrors are carried by every place that rebuilds a list (transport_far, vf_engine_compact, vf_engine_grow).
    // On the device the two arrays are late: the first list that carries a loss other than VF_LOSS_NONE moves the records of x_in into
    // an allocation with room for them behind the records (vf::far_loss_words) and sets View::x_loss, from where on k_linearize_extra
    // is the instance that reads them -- another launch sequence, so a captured one is void.  An engine that never saw a far loss
    // allocates, copies and launches what it always has.
    std::vector<std::vector<int>> h_xloss;
    std::vector<std::vector<double>> h_xk;
    vf::DeviceBuf<double> x_li_loss;
    double* x_loss_k(int window) const { return v.x_in + vf::far_loss_k_at((size_t)v.B * x_cap) + (size_t)window * x_cap; }
    int* x_loss_id(int window) const { return (int*)(v.x_in + vf::far_loss_id_at((size_t)v.B * x_cap)) + (size_t)window * x_cap; }
    int ensure_far_loss() {          // after attach_far
        if (v.x_loss) return VF_OK;
        const size_t n = (size_t)v.B * x_cap, rec_bytes = n * vf::BTW_IN * sizeof(double), all = vf::far_loss_words(n) * sizeof(double);
        HIPCHK(x_li_loss.ensure(all));
        HIPCHK(hipMemcpyAsync(x_li_loss, x_li, rec_bytes, hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemsetAsync((char*)x_li_loss.get() + rec_bytes, 0, all - rec_bytes, stream));
        x_li = x_li_loss;            // (the records' first home stays in the engine's arena, unused)
        v.x_in = x_li;
        v.x_loss = 1;
        epoch++;
        return VF_OK;
    }
    vf::DeviceBuf<double> x_gtmp;
    vf::DeviceBuf<double> x_Z;   // 6 columns of x_zstride for every slot in use; grown on demand, never beyond x_cap slots
    size_t x_zstride = 0;
    int x_cap = VF_MAX_EXTRA;  // far factors a window may hold (vf_engine_opts.max_far_factors): the width of the device lists
    // the device lists are allocated once (they stay in `allocs`); a failure half way leaves what exists in place and a
    // later call picks up from there (no second allocation, nothing leaked)
    int *x_la = nullptr, *x_lb = nullptr;
    double *x_li = nullptr, *x_lo = nullptr;
    // Woodbury columns of a single-window engine as one batch: a second engine of up to 6 x x_cap windows and the same
    // capacity, on this engine's stream; window q holds a copy of the window's H and column q of U as right-hand side
    // (k_cols_prepare), one partitioned solve of it returns all of Z.  Made when the first far factor arrives, never inside a
    // solve (a solve may be under stream capture); absent (sequential columns, as on batch engines) if it cannot be had.
    vf_engine* far_columns = nullptr;
    bool is_far_columns = false;
    bool far_columns_off = false;   // a column engine could not be made: the columns are solved one after the other
                                    // (with the arrays, so a grown engine tries again: ADVICE round 6, "far_columns_off is not carried")
    // linear far factors (View::xl_*; made and kept by k_marginalize): the host mirrors only their number and far ends
    std::vector<std::vector<int>> h_lb;
    int h_ln(int w) const { return h_lb.empty() ? 0 : (int)h_lb[w].size(); }
    void attach_far() {              // after ensure_far: the View sees the slot arrays, the host mirrors exist
        if (v.x_max) return;
        v.x_a = x_la; v.x_b = x_lb; v.x_in = x_li; v.x_out = x_lo;
        v.x_max = x_cap;
        v.far_big = tune.far_big_forms && x_cap > vf::MAX_EXTRA ? 1 : 0;
        h_xn.assign(v.B, 0);
        h_xdirty.assign(v.B, 1);
        h_xa.assign(v.B, {});
        h_xb.assign(v.B, {});
        h_xrec.assign(v.B, {});
        h_xloss.assign(v.B, {});
        h_xk.assign(v.B, {});
        h_lb.assign(v.B, {});
    }
    void recount_far() {
        x_used = 0;
        for (int w = 0; w < v.B && v.x_max; w++) x_used = std::max(x_used, h_xn[w] + h_ln(w));
    }
    int ensure_far(int slots) {
        const size_t B = (size_t)v.B, X = (size_t)x_cap;
        int rc;
        if (!x_la) { if ((rc = alloc(&x_la, B * X, false))) return rc; HIPCHK(hipMemsetAsync(x_la, 0xff, B * X * sizeof(int), stream)); }
        if (!x_lb) { if ((rc = alloc(&x_lb, B * X, false))) return rc; HIPCHK(hipMemsetAsync(x_lb, 0xff, B * X * sizeof(int), stream)); }
        if (!x_li && (rc = alloc(&x_li, B * X * vf::BTW_IN))) return rc;
        if (!x_lo && (rc = alloc(&x_lo, 2 * B * X * vf::BTW_OUT))) return rc;
        if ((!v.xl_n && (rc = alloc(&v.xl_n, B))) || (!v.xl_b && (rc = alloc(&v.xl_b, B * X))) || (!v.xl_U && (rc = alloc(&v.xl_U, B * X * 6 * (27 + 6 * X)))) ||
            (!v.xl_r0 && (rc = alloc(&v.xl_r0, B * X * 6))) || (!v.xl_bx && (rc = alloc(&v.xl_bx, B * X * 7))) || (!v.xl_out && (rc = alloc(&v.xl_out, 2 * B * X * 6)))) return rc;
        // (more far factors than the LDS forms of k_marginalize / k_extra_combine hold: their systems live here)
        // (the others: room for the solution of the Woodbury system, handed from k_extra_combine to k_extra_apply)
        if (!v.far_scratch && (rc = alloc(&v.far_scratch, B * (x_cap > vf::MAX_EXTRA ? vf::FAR_SCRATCH : (size_t)64)))) return rc;
        x_zstride = (size_t)v.G * 15 + B + 64;
        HIPCHK(x_gtmp.ensure(x_zstride * sizeof(double)));
        const size_t zbytes = 6 * (size_t)slots * x_zstride * sizeof(double);
        if (zbytes > x_Z.bytes()) {
            // the solved columns of the low-rank correction: 6 increment-shaped columns per slot IN USE (one far factor in
            // one window of a 1024 x 1088 batch engine is 0.8 GB, not the 6.4 GB that VF_MAX_EXTRA slots would be)
            HIPCHK(hipStreamSynchronize(stream));
            HIPCHK(x_Z.ensure(zbytes));
        }
        return VF_OK;
    }
    // refined solve (vf_refine.hip): work vectors, allocated on first use; refine_open: a time-sharded caller is between
    // vf_engine_refine_begin and vf_engine_refine_end, and vf_engine_solve_local / _global work on (nres, z)
    vf::Refine rq{};
    bool rq_ready = false, refine_open = false;
    vf::PinnedBuf<int> rq_stop_host;     // [B] pinned: the stop flags, read back between corrections (vf_engine_solve)
    int ensure_refine() {
        if (rq_ready) return VF_OK;
        const size_t G = (size_t)v.G, B = (size_t)v.B;
        int rc;
        HIPCHK(rq_stop_host.ensure(B * sizeof(int)));
        if ((rc = alloc(&rq.x, G * 15)) || (rc = alloc(&rq.p, G * 15)) || (rc = alloc(&rq.Ap, G * 15)) ||
            (rc = alloc(&rq.nres, G * 15 + 64)) || (rc = alloc(&rq.z, G * 15 + B)) || (rc = alloc(&rq.u_imu, G * 15)) ||
            (rc = alloc(&rq.u_btw, G * 6)) || (rc = alloc(&rq.u_pri, B * 15)) || (rc = alloc(&rq.rz, B)) ||
            (rc = alloc(&rq.rz0, B)) || (rc = alloc(&rq.stop, B)) || (rc = alloc(&rq.iters, B)) ||
            (rc = alloc(&rq.part, B * 64)) || (rc = alloc(&rq.coef, B)) || (rc = alloc(&rq.first, B))) return rc;
        rq_ready = true;
        return VF_OK;
    }
    // corrections per solve: vf_engine_opts.refine_iterations, or (auto) 12 once a window is longer than refine_min_keyframes
    int refine_iters() const {
        if (opts.refine_iterations >= 0) return opts.refine_iterations;
        int longest = 0;
        for (int w = 0; w < v.B; w++) longest = std::max(longest, h_hi[w] - h_lo[w]);
        return longest > opts.refine_min_keyframes ? 12 : 0;
    }
    // ... and how far each solve's corrections are driven (auto mode).  What the normal equations get wrong grows smoothly with
    // the window -- plain Gauss-Newton contracts by 0.1 per update at 1 500 keyframes, 0.3 at 2 000, 0.7 at 3 000 -- so the
    // residual reduction a solve is refined to tightens smoothly too, from 1e-3 where refinement starts to refine_rel_stop at
    // twice that length: 1-2 corrections just above the threshold instead of 4, 5 at 3 000 as before (round 5's switch from
    // none to "until 1e-8" made vf_solve four times dearer between 1 500 and 1 600 keyframes).
    double refine_stop() const {
        if (opts.refine_iterations >= 0 || !(opts.refine_rel_stop < 1e-3)) return opts.refine_rel_stop;
        int longest = 0;
        for (int w = 0; w < v.B; w++) longest = std::max(longest, h_hi[w] - h_lo[w]);
        const double n0 = opts.refine_min_keyframes, n1 = 2.0 * n0;
        if (longest >= n1 || n0 <= 0) return opts.refine_rel_stop;
        const double t = std::max(0.0, (longest - n0) / (n1 - n0));
        return std::pow(10.0, -3.0 + t * (std::log10(opts.refine_rel_stop) + 3.0));
    }
    // non-monotone LM (vf_engine_opts.lm_excursion): provisional trials allowed per excursion; auto = 3 on engines that refine
    int excursion() const { return opts.lm_excursion >= 0 ? opts.lm_excursion : (refine_iters() > 0 ? 3 : 0); }
    int ensure_excursion() {
        if (v.x_best) return VF_OK;
        int rc;
        if ((rc = alloc(&v.x_best, 16 * (size_t)v.G)) || (rc = alloc(&v.ref_cost, (size_t)v.B)) || (rc = alloc(&v.prov, (size_t)v.B)) ||
            (rc = alloc(&v.n_prov, (size_t)v.B)) || (rc = alloc(&v.relin, (size_t)v.B)) || (rc = alloc(&v.carry, (size_t)v.B))) return rc;
        return VF_OK;
    }
    // marginal covariances (engine/engine_marginals.inc): [G][SIG_SLOT] blocks + per-window failure flags, a zero lambda and
    // all-ones `fresh` flags for the undamped factorisation, one allocation made by the first vf_engine_marginals.  What of all
    // this is there to be read is SolveMemory's to say (covariances_valid, pose_records_valid, score_rows); sig_lo / sig_hi: the
    // ranges the blocks were computed for, read only behind covariances_valid()
    vf::DeviceBuf<double> sig;
    double* sig_zero() const { return sig + (size_t)v.G * vf::SIG_SLOT; }
    int* sig_fail() const { return (int*)(sig_zero() + v.B); }
    int* sig_ones() const { return sig_fail() + v.B; }
    std::vector<int> sig_lo, sig_hi;
    // vf_engine_marginals_ex with VF_MARGINALS_FAR: Z = A^-1 U and the m x m systems of a group of windows (vf::FarCov), allocated
    // on first use and grown when a later call needs more; FARCOV_BUDGET bounds it, more windows than fit are done in groups
    vf::DeviceBuf<double> fc_scratch;
    // VF_MARGINALS_POSE (kernels/kpose.inc): the pose marginals in nav_msgs order, their inverses and the poses, [G][36], [G][36] and
    // [G][6] in one allocation made by the first call that carries the flag, with the range [B][2] each window's records are of
    vf::DeviceBuf<double> pm_cov;
    double* pm_info() const { return pm_cov + (size_t)v.G * 36; }
    double* pm_pose() const { return pm_cov + (size_t)v.G * 72; }
    int* pm_range() const { return (int*)(pm_cov + (size_t)v.G * 78); }
    // vf_engine_marginal_scores: one row of G scores per subset asked for, grown on demand
    vf::DeviceBuf<double> sc;
    // vf_engine_factor_errors (engine/engine_errors.inc): [G] + [G] errors of the band factors, [B][2 x_cap] of the far factors, the
    // windows' summaries and the batch's block, one allocation made by the first call.  Whether it holds anything is SolveMemory's
    // to say (errors_valid); err_lo / err_hi: the ranges the call saw, read only behind errors_valid()
    vf::DeviceBuf<double> err;
    static_assert(sizeof(vf::ErrSummary) % sizeof(double) == 0 && sizeof(vf::ErrSummary) == sizeof(vf_consistency), "vf_consistency and its device twin");
    static_assert(sizeof(vf::BatchHealth) == sizeof(vf_batch_health), "vf_batch_health and its device twin");
    vf::FactorErrors err_view() const {
        vf::FactorErrors o{};
        o.imu = err;
        o.btw = err + (size_t)v.G;
        o.far = err + 2 * (size_t)v.G;
        o.summary = (vf::ErrSummary*)(o.far + (size_t)v.B * 2 * x_cap);
        o.health = (vf::BatchHealth*)(o.summary + v.B);
        o.x_cap = x_cap;
        return o;
    }
    size_t err_bytes() const { return (2 * (size_t)v.G + (size_t)v.B * 2 * x_cap) * sizeof(double) + (size_t)v.B * sizeof(vf::ErrSummary) + sizeof(vf::BatchHealth); }
    std::vector<int> err_lo, err_hi;
    // robust losses of the band between factors (engine/engine_robust.inc; View::btw_loss, btw_loss_k): [G] ids and [G] parameters,
    // made by the first vf_engine_set_between_loss that sets a loss other than VF_LOSS_NONE.  From then on the K2 launches are the
    // kernels that read them -- another launch sequence, so a captured one is void
    vf::DeviceBuf<int> loss_id;
    vf::DeviceBuf<double> loss_k;
    int ensure_loss() {
        if (v.btw_loss) return VF_OK;
        HIPCHK(loss_id.ensure((size_t)v.G * sizeof(int)));
        HIPCHK(loss_k.ensure((size_t)v.G * sizeof(double)));
        HIPCHK(hipMemsetAsync(loss_id, 0, (size_t)v.G * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(loss_k, 0, (size_t)v.G * sizeof(double), stream));
        v.btw_loss = loss_id;
        v.btw_loss_k = loss_k;
        epoch++;
        return VF_OK;
    }
    // absolute factors in the between slot (engine/engine_absolute.inc): [G] kinds, VF_ABSOLUTE_*, made by the first
    // vf_engine_set_absolute behind the loss arrays (the kernels that read kinds read losses).  Not a member of View, whose 712
    // bytes have no word left: btw_kind is handed to the launchers, which choose the K2 kernels by it -- another launch sequence
    // from then on, so a captured one is void
    vf::DeviceBuf<int> kind_id;
    int* btw_kind = nullptr;
    int ensure_kind() {
        if (btw_kind) return VF_OK;
        if (int rc = ensure_loss()) return rc;
        HIPCHK(kind_id.ensure((size_t)v.G * sizeof(int)));
        HIPCHK(hipMemsetAsync(kind_id, 0, (size_t)v.G * sizeof(int), stream));
        btw_kind = kind_id;
        epoch++;
        return VF_OK;
    }
    // NONE for the slots [g0, g0 + n) whose record a staging call has just written or cleared: their loss and their kind (nothing on
    // an engine without the arrays)
    int reset_loss(long g0, long n) {
        if (!v.btw_loss || n <= 0) return VF_OK;
        HIPCHK(hipMemsetAsync(v.btw_loss + g0, 0, (size_t)n * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(v.btw_loss_k + g0, 0, (size_t)n * sizeof(double), stream));
        if (btw_kind) HIPCHK(hipMemsetAsync(btw_kind + g0, 0, (size_t)n * sizeof(int), stream));
        return VF_OK;
    }
    // vf_engine_grow: the arrays of `o` come behind this handle (and this one's go behind o's, to be destroyed with it)
    void swap_arrays(vf_engine& o) { std::swap(*this, o), std::swap<EngineHandle>(*this, o); }
};

Entry::Entry(vf_engine* e, Effect does, int flags) : engine(e) {
    if (!e) return;
    if (!(flags & overlaps) && e->side_open) (void)e->join_side();
    e->mem.entry_ran(flags & leaves_result);
    if (does.kind == 2) e->mem.rewritten();
    else if (does.kind == 1) e->mem.written_from(does.window, does.slot, e->h_lo[0], e->h_hi[0]);
    want = e->opts.device;
    if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipSetDevice(want); return; }
    if (prev != want) (void)hipSetDevice(want);
}

extern "C" {
#include "engine/engine_create.inc"
#include "engine/engine_staging.inc"
#include "engine/engine_solve.inc"
#include "engine/engine_shard.inc"
#include "engine/engine_misc.inc"
#include "engine/engine_compat.inc"
#include "engine/engine_window.inc"
#include "engine/engine_read.inc"
#include "engine/engine_marginals.inc"
#include "engine/engine_propagate.inc"
#include "engine/engine_gate.inc"
#include "engine/engine_closure.inc"
#include "engine/engine_errors.inc"
#include "engine/engine_robust.inc"
#include "engine/engine_absolute.inc"
}  // extern "C"
