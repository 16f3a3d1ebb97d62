// engine/engine_shard.inc -- chunk geometry, time-sharded windows, their collectives from C (RCCL by dlopen).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// ------------------------------------------------------------------ chunk geometry (host only, no device needed)
int vf_chunk_geometry(int n, int chunks, int fit, int c, int* count, int* first, int* interior, int* has_separator) {
    if (n < 0 || chunks < 1) return fail(VF_ERR_INVALID, "bad geometry query");
    const int Pe = vf::chunk_count(n, chunks, fit ? 1 : 0);
    if (count) *count = Pe;
    if (c < 0 || c >= Pe) {
        if (first || interior || has_separator) return fail(VF_ERR_INVALID, "chunk %d out of range (%d)", c, Pe);
        return VF_OK;
    }
    const vf::ChunkGeom g = vf::chunk_geom(n, Pe, c);
    if (first) *first = g.i0;
    if (interior) *interior = g.ni;
    if (has_separator) *has_separator = g.has_sep;
    return VF_OK;
}
int vf_shard_range(int n, int chunks, int fit, int rank, int world, int* chunk_lo, int* chunk_hi, int* kf_lo, int* kf_hi) {
    if (n < 0 || chunks < 1 || world < 1 || rank < 0 || rank >= world) return fail(VF_ERR_INVALID, "bad shard query");
    const int Pe = vf::chunk_count(n, chunks, fit ? 1 : 0);
    const int c0 = (int)((long)rank * Pe / world), c1 = (int)((long)(rank + 1) * Pe / world);
    if (chunk_lo) *chunk_lo = c0;
    if (chunk_hi) *chunk_hi = c1;
    if (kf_lo) *kf_lo = c0 < Pe ? vf::chunk_geom(n, Pe, c0).i0 : n;
    if (kf_hi) *kf_hi = c1 < Pe ? vf::chunk_geom(n, Pe, c1).i0 : n;
    return VF_OK;
}

// ------------------------------------------------------------------ time-sharded windows (multi-GPU)
int vf_engine_set_stream(vf_engine* e, void* hip_stream) {
    VF_ENTER(e, Entry::rewrites);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->own_stream && e->stream) HIPCHK(hipStreamDestroy(e->stream));
    e->drop_graph();
    e->stream = (hipStream_t)hip_stream;      // nullptr = the device's default stream
    e->own_stream = false;
    if (e->far_columns) return vf_engine_set_stream(e->far_columns, hip_stream);
    return VF_OK;
}
int vf_engine_set_shard(vf_engine* e, int rank, int world) {
    VF_ENTER(e, Entry::rewrites);
    if (world < 1 || rank < 0 || rank >= world) return fail(VF_ERR_INVALID, "bad shard %d of %d", rank, world);
    if (world > 1 && (e->v.P < 2 || e->v.P_fit))
        return fail(VF_ERR_INVALID, "time sharding needs an explicit chunk count (vf_engine_opts.chunks >= 2)");
    if (world > 1 && e->v.P % world != 0) return fail(VF_ERR_INVALID, "chunks (%d) must be a multiple of the world size (%d)", e->v.P, world);
    if (world > 1 && e->v.btw_loss) return fail(VF_ERR_INVALID, "this engine holds robust losses (vf_engine_set_between_loss): losses on time-sharded engines are not built");
    if (world > 1 && e->v.x_loss) return fail(VF_ERR_INVALID, "this engine holds robust losses of far factors (vf_engine_set_extra_between_robust): losses on time-sharded engines are not built");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->v.sh_r = rank;
    e->v.sh_G = world;
    e->mem.sharded = world > 1;
    e->epoch++;
    return VF_OK;
}
int vf_engine_shard_info(vf_engine* e, vf_shard_info* out) {
    Entry entry_(e, Entry::reads);
    if (!e || !out) return fail(VF_ERR_INVALID, "null argument");
    if (e->v.P < 2) return fail(VF_ERR_INVALID, "engine was not created with the partitioned solve (chunks >= 2)");
    memset(out, 0, sizeof(*out));
    out->rank = e->v.sh_r; out->world = e->v.sh_G; out->windows = e->v.B; out->chunks = e->v.P;
    out->sep = e->v.sepR;
    out->sep_per_chunk = (long)e->v.B * vf::SEPK;
    out->delta = e->v.delta; out->delta_count = e->v.G * 15 + e->v.B;
    // (the refinement's work vectors only for engines that refine as their windows stand NOW: ask again after loading longer ones)
    if (e->refine_iters() > 0) {
        if (int rc = e->ensure_refine()) return rc;
        HIPCHK(hipStreamSynchronize(e->stream));
        out->refine_delta = e->rq.z;
    }
    return VF_OK;
}
// what the staged solve works on: the engine's system, or while a refinement is open the correction's (converged windows are skipped)
static vf::View staged_view(const vf_engine* e) {
    return e->refine_open ? vf::on_buffers(e->v, e->rq.nres, e->rq.z, e->rq.stop) : e->v;
}
static int check_sharded(vf_engine* e) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (e->v.P < 2) return fail(VF_ERR_INVALID, "engine was not created with the partitioned solve (chunks >= 2)");
    if (e->v.sh_G > 1)
        for (int w = 0; w < e->v.B; w++) {
            const int n = e->h_hi[w] - e->h_lo[w];
            if (n > 0 && vf::chunk_count(n, e->v.P, e->v.P_fit) != e->v.P)
                return fail(VF_ERR_INVALID, "window %d (%d keyframes) is too short for %d chunks", w, n, e->v.P);
        }
    return VF_OK;
}
int vf_engine_solve_local(vf_engine* e) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_sharded(e);
    if (rc) return rc;
    vf::launch_partitioned_local(staged_view(e), e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
int vf_engine_solve_global(vf_engine* e) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_sharded(e);
    if (rc) return rc;
    const vf::View a = staged_view(e);
    vf::launch_partitioned_global(a, e->stream);
    if (e->v.sh_G > 1) vf::launch_mask_delta(a, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
// ------------------------------------------------------------------ the collectives of a time-sharded window from C (RCCL)
// A C / C++ caller (the reference's node is C++) cannot reach torch.distributed: here the library issues the two collectives
// of a solve itself, on the engine's stream, through the communicator the caller hands in (ncclComm_t; created by the caller
// with ncclCommInitRank / ncclCommInitAll).  librccl is looked up at run time (dlopen): libvilfusion.so itself keeps no
// communication dependency, and a process that never calls these entry points never loads it.
namespace {
typedef int (*rccl_all_gather_t)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*rccl_all_reduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*rccl_error_string_t)(int);
struct Rccl {
    void* handle = nullptr;
    rccl_all_gather_t all_gather = nullptr;
    rccl_all_reduce_t all_reduce = nullptr;
    rccl_error_string_t error_string = nullptr;
    bool tried = false;
};
Rccl g_rccl;
constexpr int RCCL_FLOAT64 = 8, RCCL_SUM = 0;      // ncclFloat64, ncclSum (rccl.h)
std::once_flag g_rccl_once;
std::string g_rccl_why;
int rccl_load() {
    // (two engines on two threads may ask at once: the library is opened by one of them)
    std::call_once(g_rccl_once, [] {
        g_rccl.tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            g_rccl.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (g_rccl.handle) break;
        }
        if (g_rccl.handle) {
            g_rccl.all_gather = (rccl_all_gather_t)dlsym(g_rccl.handle, "ncclAllGather");
            g_rccl.all_reduce = (rccl_all_reduce_t)dlsym(g_rccl.handle, "ncclAllReduce");
            g_rccl.error_string = (rccl_error_string_t)dlsym(g_rccl.handle, "ncclGetErrorString");
        }
        if (!g_rccl.all_gather || !g_rccl.all_reduce) {
            const char* why = dlerror();
            g_rccl_why = why ? why : "symbols missing";
        }
    });
    if (!g_rccl.all_gather || !g_rccl.all_reduce)
        return fail(VF_ERR_DEVICE, "librccl not found (dlopen librccl.so.1): %s", g_rccl_why.c_str());
    return VF_OK;
}
int rccl_check(int rc, const char* what) {
    if (rc == 0) return VF_OK;
    return fail(VF_ERR_DEVICE, "%s failed: %s", what, g_rccl.error_string ? g_rccl.error_string(rc) : "rccl error");
}
// one staged solve of the shard: local phase, all-gather of the packed separator system (in place: the rank's own slice of
// the receive buffer is its send buffer), global phase, all-reduce of increments + failure flags; then the refinement, each
// correction the same two collectives on the correction's buffers
int shard_solve(vf_engine* e, void* comm) {
    int rc;
    const vf::View& v = e->v;
    const size_t per_chunk = (size_t)v.B * vf::SEPK, per_rank = (size_t)(v.P / v.sh_G) * per_chunk;
    const size_t nd = (size_t)v.G * 15 + (size_t)v.B;
    auto exchange = [&](double* delta) -> int {
        int r;
        if ((r = vf_engine_solve_local(e))) return r;
        if ((r = rccl_check(g_rccl.all_gather(v.sepR + (size_t)v.sh_r * per_rank, v.sepR, per_rank, RCCL_FLOAT64, comm, e->stream), "ncclAllGather"))) return r;
        if ((r = vf_engine_solve_global(e))) return r;
        return rccl_check(g_rccl.all_reduce(delta, delta, nd, RCCL_FLOAT64, RCCL_SUM, comm, e->stream), "ncclAllReduce");
    };
    if ((rc = vf_engine_assemble(e)) || (rc = exchange(e->v.delta))) return rc;
    int R = 0;
    if ((rc = vf_engine_refine_count(e, &R))) return rc;
    if (R > 0) {
        if ((rc = vf_engine_refine_begin(e))) return rc;
        for (int it = 0; it < R; it++)
            if ((rc = exchange(e->rq.z)) || (rc = vf_engine_refine_step(e))) {
                e->refine_open = false;       // (a failed collective must not leave later solves on the correction's buffers)
                return rc;
            }
        if ((rc = vf_engine_refine_end(e))) { e->refine_open = false; return rc; }
    }
    return VF_OK;
}
int shard_ready(vf_engine* e, void* comm, const char* what) {
    if (!e || !comm) return fail(VF_ERR_INVALID, "%s: null argument", what);
    if (e->v.P < 2 || e->v.P_fit) return fail(VF_ERR_INVALID, "%s: the engine needs an explicit chunk count (vf_engine_opts.chunks >= 2) and vf_engine_set_shard", what);
    return rccl_load();
}
}  // namespace

int vf_shard_exchange_plan(int windows, int capacity, int chunks, int rank, int world, long* sep_offset, long* sep_count,
                           long* sep_total, long* delta_count) {
    if (windows < 1 || capacity < 1 || chunks < 2 || world < 1 || rank < 0 || rank >= world || chunks % world != 0)
        return fail(VF_ERR_INVALID, "bad exchange-plan query");
    const long M = (capacity + 63) / 64 * 64, per_chunk = (long)windows * vf::SEPK, per_rank = (long)(chunks / world) * per_chunk;
    if (sep_offset) *sep_offset = rank * per_rank;
    if (sep_count) *sep_count = per_rank;
    if (sep_total) *sep_total = (long)chunks * per_chunk;
    if (delta_count) *delta_count = (long)windows * M * 15 + windows;
    return VF_OK;
}
int vf_shard_iterate(vf_engine* e, void* nccl_comm, int iterations) {
    Entry entry_(e, Entry::reads);
    int rc = shard_ready(e, nccl_comm, "vf_shard_iterate");
    if (rc) return rc;
    if (iterations < 0) return fail(VF_ERR_INVALID, "iterations < 0");
    if ((rc = vf_engine_reset_lambda(e)) || (rc = vf_engine_linearize(e, 0)) || (rc = vf_engine_decide(e, 1))) return rc;
    for (int it = 0; it < iterations; it++)
        if ((rc = shard_solve(e, nccl_comm)) || (rc = vf_engine_retract(e)) || (rc = vf_engine_linearize(e, 1)) || (rc = vf_engine_decide(e, 0))) return rc;
    if (iterations > 0 && (rc = vf_engine_close_excursions(e))) return rc;
    return VF_OK;
}
int vf_shard_gn_step(vf_engine* e, void* nccl_comm, double relin_threshold) {
    Entry entry_(e, Entry::reads);
    int rc = shard_ready(e, nccl_comm, "vf_shard_gn_step");
    if (rc) return rc;
    if ((rc = vf_engine_gn_begin(e, relin_threshold)) || (rc = shard_solve(e, nccl_comm)) || (rc = vf_engine_retract(e))) return rc;
    return VF_OK;
}
