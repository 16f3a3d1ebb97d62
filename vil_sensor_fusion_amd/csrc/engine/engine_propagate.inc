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
    if (int rc = not_sharded(e, "vf_engine_propagate_tail")) return rc;
    const bool cov = (flags & VF_PROPAGATE_COVARIANCE) != 0;
    const int B = e->v.B;
    const int total = step_off[B];
    if (step_off[0] != 0 || (total > 0 && !steps)) return fail(VF_ERR_INVALID, "bad step offsets");
    if (cov && !e->mem.covariances_valid())
        return fail(VF_ERR_INVALID, "vf_engine_propagate_tail: VF_PROPAGATE_COVARIANCE needs the marginal covariances of the last keyframes: call vf_engine_marginals_ex first");
    for (int w = 0; w < B; w++) {
        if (step_off[w + 1] < step_off[w]) return fail(VF_ERR_INVALID, "bad step offsets (window %d)", w);
        const int hi = e->h_hi[w], lo = e->h_lo[w];
        if (hi <= lo) return fail(VF_ERR_BAD_KEY, "window %d is empty", w);
        if (cov && (hi - 1 < e->sig_lo[w] || hi > e->sig_hi[w]))
            return fail(VF_ERR_INVALID, "vf_engine_propagate_tail: window %d: the covariances were computed for the keyframes [%d,%d), the last keyframe is %d",
                        w, e->sig_lo[w], e->sig_hi[w], hi - 1);
    }
    // one packed block: [offsets B + 1][steps 7 x total]
    const size_t off_b = ((size_t)(B + 1) * sizeof(int) + 7) & ~(size_t)7, st_b = (size_t)total * 7 * sizeof(double);
    const size_t bytes = off_b + st_b;
    if (!e->prop_ev[0])
        for (auto& ev : e->prop_ev) HIPCHK(hipEventCreate(&ev));
    if (bytes > e->prop_host.bytes() || bytes > e->prop_dev.bytes()) {
        if (e->prop_pending) HIPCHK(hipEventSynchronize(e->prop_ev[2]));      // (the copy out of, and the kernel on, the blocks about to go)
        HIPCHK(e->prop_host.ensure(bytes, vf::twice));
        HIPCHK(e->prop_dev.ensure(bytes, vf::twice));
    }
    HIPCHK(e->prop_out.ensure((size_t)B * (16 + 225) * sizeof(double)));
    if (e->prop_pending) HIPCHK(hipEventSynchronize(e->prop_ev[1]));          // the previous call's copy has left the pinned buffer: long done
    char* h = e->prop_host;
    memcpy(h, step_off, (size_t)(B + 1) * sizeof(int));
    if (total > 0) memcpy(h + off_b, steps, st_b);
    char* d = e->prop_dev;
    HIPCHK(hipEventRecord(e->prop_ev[0], e->stream));
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->prop_ev[1], e->stream));
    vf::ImuCov c{p->acc_cov, p->gyro_cov, p->integration_cov, p->bias_acc_cov, p->bias_omega_cov, p->bias_acc_omega_int};
    vf::launch_propagate(e->v, (const int*)d, (const double*)(d + off_b), c, cov ? 1 : 0, (flags & VF_PROPAGATE_FROM_ESTIMATE) ? 1 : 0,
                         cov ? e->sig.get() : nullptr, cov ? e->sig_fail() : nullptr, e->prop_out, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->prop_ev[2], e->stream));
    e->prop_pending = true;
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
    if (h2d_ms) *h2d_ms = 0.f;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!e->prop_pending) return VF_OK;
    HIPCHK(hipEventSynchronize(e->prop_ev[2]));
    if (h2d_ms) HIPCHK(hipEventElapsedTime(h2d_ms, e->prop_ev[0], e->prop_ev[1]));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, e->prop_ev[1], e->prop_ev[2]));
    return VF_OK;
}
