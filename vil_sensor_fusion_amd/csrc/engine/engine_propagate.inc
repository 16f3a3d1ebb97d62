// engine/engine_propagate.inc -- the state between two solves, at IMU rate, with its propagated covariance
// (vf_engine_propagate_tail / vf_engine_read_propagated / vf_engine_propagate_status; kernels/kprop.inc).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.
//
// One pinned copy and one launch on the engine's stream, no host synchronisation.  The call writes its own buffer and nothing
// else: states, records, linearisations, lambda, counters, sticky words, the far lists, the stash and the cached result block
// are as they were, and so is everything SolveMemory knows but the one fact that a propagation exists.
int vf_engine_propagate_tail(vf_engine* e, const int32_t* step_off, const double* steps, const vf_imu_params* p, unsigned flags) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (!e || !step_off || !p) return fail(VF_ERR_INVALID, "null argument");
    if (flags & ~(unsigned)(VF_PROPAGATE_COVARIANCE | VF_PROPAGATE_FROM_ESTIMATE)) return fail(VF_ERR_INVALID, "vf_engine_propagate_tail: unknown flags 0x%x", flags);
    const bool cov = (flags & VF_PROPAGATE_COVARIANCE) != 0;
    const int B = e->v.B;
    if (int rc = check_tail_steps(e, "vf_engine_propagate_tail", step_off, steps, !cov ? nullptr :
                                  "VF_PROPAGATE_COVARIANCE needs the marginal covariances of the last keyframes: call vf_engine_marginals_ex first")) return rc;
    // one packed block: [offsets B + 1][steps 7 x total]
    vf::Packed blk;
    const size_t st_b = (size_t)step_off[B] * 7 * sizeof(double), off_at = blk.add((size_t)(B + 1) * sizeof(int)), st_at = blk.add(st_b);
    HIPCHK(e->prop_out.ensure((size_t)B * (16 + 225) * sizeof(double)));
    char* h = nullptr;
    HIPCHK(e->prop.open(blk.bytes, &h));
    memcpy(h + off_at, step_off, (size_t)(B + 1) * sizeof(int));
    if (st_b > 0) memcpy(h + st_at, steps, st_b);
    HIPCHK(e->prop.send(blk.bytes, e->stream, true));
    const char* d = e->prop.device();
    vf::launch_propagate(e->v, (const int*)(d + off_at), (const double*)(d + st_at), imu_cov(p), cov ? 1 : 0, (flags & VF_PROPAGATE_FROM_ESTIMATE) ? 1 : 0,
                         cov ? e->sig.get() : nullptr, cov ? e->sig_fail() : nullptr, e->prop_out, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(e->prop.launched(e->stream));
    e->mem.propagated(cov);
    return VF_OK;
}

int vf_engine_read_propagated(vf_engine* e, int window, double* state16, double* cov225) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (int rc = check_window(e, window)) return rc;
    if (!e->mem.propagation_valid())
        return fail(VF_ERR_INVALID, "vf_engine_read_propagated: no propagation since the engine was made or grown: call vf_engine_propagate_tail first");
    if (cov225 && !e->mem.propagated_covariance_valid())
        return fail(VF_ERR_INVALID, "vf_engine_read_propagated: the last vf_engine_propagate_tail did not carry VF_PROPAGATE_COVARIANCE");
    const double* src = e->prop_out + (size_t)window * (16 + 225);
    if (state16) HIPCHK(hipMemcpyAsync(state16, src, 16 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (cov225) HIPCHK(hipMemcpyAsync(cov225, src + 16, 225 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_propagate_status(vf_engine* e, float* h2d_ms, float* kernel_ms) {
    VF_ENTER(e, Entry::reads, Entry::leaves_result);
    HIPCHK(e->prop.timings(h2d_ms, kernel_ms));
    return VF_OK;
}
