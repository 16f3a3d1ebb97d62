// engine/engine_gate.inc -- the innovation gate: chi-square of an incoming between factor against the window as solved and the IMU
// since, before the factor is added (vf_engine_gate_tail / vf_engine_read_gate / vf_engine_read_gate_all / vf_engine_gate_status;
// kernels/kgate.inc).  A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside
// extern "C", never compiled by itself.
//
// One pinned copy and one launch on the engine's stream, no host synchronisation, as vf_engine_propagate_tail -- from buffers of this
// call's own (the propagation's and the ingest's may be in flight).  The call writes its own result buffer and nothing else: states,
// records, linearisations, lambda, counters, sticky words, the far lists, the stash, the covariances, the propagation, the factor
// errors and the cached result block are as they were, and so is everything SolveMemory knows but the one fact that a gate result
// exists.  The covariances are read as the last vf_engine_marginals_ex left them: a far downdate is honoured for free.
static_assert(sizeof(vf_gate_result) == vf::GATE_RECORD, "vf_gate_result and its device twin (kernels/kgate.inc)");
int vf_engine_gate_tail(vf_engine* e, const int32_t* step_off, const double* steps, const vf_imu_params* p, const int32_t* btw_a,
                        const double* btw_rec28, double chi2_threshold, unsigned flags) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (!e || !step_off || !p || !btw_a || !btw_rec28) return fail(VF_ERR_INVALID, "null argument");
    if (flags & ~(unsigned)VF_GATE_FROM_ESTIMATE) return fail(VF_ERR_INVALID, "vf_engine_gate_tail: unknown flags 0x%x", flags);
    if (int rc = not_sharded(e, "vf_engine_gate_tail")) return rc;
    const int B = e->v.B;
    const int total = step_off[B];
    if (step_off[0] != 0 || (total > 0 && !steps)) return fail(VF_ERR_INVALID, "bad step offsets");
    if (!e->mem.covariances_valid())
        return fail(VF_ERR_INVALID, "vf_engine_gate_tail: needs the marginal covariances of the last keyframes: call vf_engine_marginals_ex first (VF_MARGINALS_TAIL is enough)");
    for (int w = 0; w < B; w++) {
        if (step_off[w + 1] < step_off[w]) return fail(VF_ERR_INVALID, "bad step offsets (window %d)", w);
        const int hi = e->h_hi[w], lo = e->h_lo[w];
        if (hi <= lo) return fail(VF_ERR_BAD_KEY, "window %d is empty", w);
        if (hi - 1 < e->sig_lo[w] || hi > e->sig_hi[w])
            return fail(VF_ERR_INVALID, "vf_engine_gate_tail: window %d: the covariances were computed for the keyframes [%d,%d), the last keyframe is %d",
                        w, e->sig_lo[w], e->sig_hi[w], hi - 1);
    }
    // one packed block: [offsets B + 1][btw_a B][first slot the covariances cover B] | [records 28 x B][steps 7 x total]
    const size_t int_b = ((size_t)(3 * B + 1) * sizeof(int) + 7) & ~(size_t)7, rec_b = (size_t)B * vf::BTW_IN * sizeof(double);
    const size_t st_b = (size_t)total * 7 * sizeof(double);
    const size_t bytes = int_b + rec_b + st_b;
    if (!e->gate_ev[0])
        for (auto& ev : e->gate_ev) HIPCHK(hipEventCreate(&ev));
    if (bytes > e->gate_host.bytes() || bytes > e->gate_dev.bytes()) {
        if (e->gate_pending) HIPCHK(hipEventSynchronize(e->gate_ev[2]));      // (the copy out of, and the kernel on, the blocks about to go)
        HIPCHK(e->gate_host.ensure(bytes, vf::twice));
        HIPCHK(e->gate_dev.ensure(bytes, vf::twice));
    }
    if (!e->gate_out) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->gate_out.ensure((size_t)B * vf::GATE_RECORD));
    }
    if (e->gate_pending) HIPCHK(hipEventSynchronize(e->gate_ev[1]));          // the previous call's copy has left the pinned buffer: long done
    char* h = e->gate_host;
    int* hi32 = (int*)h;
    memcpy(hi32, step_off, (size_t)(B + 1) * sizeof(int));
    memcpy(hi32 + B + 1, btw_a, (size_t)B * sizeof(int));
    memcpy(hi32 + 2 * B + 1, e->sig_lo.data(), (size_t)B * sizeof(int));
    memcpy(h + int_b, btw_rec28, rec_b);
    if (total > 0) memcpy(h + int_b + rec_b, steps, st_b);
    char* d = e->gate_dev;
    const int* d32 = (const int*)d;
    HIPCHK(hipEventRecord(e->gate_ev[0], e->stream));
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->gate_ev[1], e->stream));
    vf::ImuCov c{p->acc_cov, p->gyro_cov, p->integration_cov, p->bias_acc_cov, p->bias_omega_cov, p->bias_acc_omega_int};
    const double thr = std::isfinite(chi2_threshold) && chi2_threshold > 0.0 ? chi2_threshold : INFINITY;
    vf::launch_gate_between(e->v, d32, (const double*)(d + int_b + rec_b), c, d32 + B + 1, d32 + 2 * B + 1, (const double*)(d + int_b), thr,
                            (flags & VF_GATE_FROM_ESTIMATE) ? 1 : 0, e->sig, e->sig_fail(), e->gate_out.get(), e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->gate_ev[2], e->stream));
    e->gate_pending = true;
    e->mem.gated();
    return VF_OK;
}

static int check_gate(vf_engine* e, int window, const char* what) {
    if (int rc = check_window(e, window)) return rc;
    if (!e->mem.gate_valid())
        return fail(VF_ERR_INVALID, "%s: no gate result: call vf_engine_gate_tail first (vf_engine_compact and vf_engine_grow void it)", what);
    return VF_OK;
}

int vf_engine_read_gate(vf_engine* e, int window, vf_gate_result* out) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (int rc = check_gate(e, window, "vf_engine_read_gate")) return rc;
    if (!out) return fail(VF_ERR_INVALID, "vf_engine_read_gate: null output");
    const uint32_t n = out->struct_size;
    if (n < sizeof(uint32_t) || n > sizeof(vf_gate_result))
        return fail(VF_ERR_INVALID, "vf_engine_read_gate: struct_size = %u: this library knows sizes up to %zu (fill it with sizeof)", n, sizeof(vf_gate_result));
    vf_gate_result r;
    HIPCHK(hipMemcpyAsync(&r, e->gate_out.get() + (size_t)window * vf::GATE_RECORD, sizeof(r), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    r.struct_size = n;
    memcpy(out, &r, n);
    return VF_OK;
}

int vf_engine_read_gate_all(vf_engine* e, int32_t* status, double* nis) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (int rc = check_gate(e, 0, "vf_engine_read_gate_all")) return rc;
    const int B = e->v.B;
    std::vector<vf_gate_result> r((size_t)B);
    HIPCHK(hipMemcpyAsync(r.data(), e->gate_out.get(), (size_t)B * vf::GATE_RECORD, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int w = 0; w < B; w++) {
        if (status) status[w] = r[w].status;
        if (nis) nis[w] = r[w].nis;
    }
    return VF_OK;
}

int vf_engine_gate_status(vf_engine* e, float* h2d_ms, float* kernel_ms) {
    VF_ENTER(e, Entry::reads, Entry::leaves_result);
    if (h2d_ms) *h2d_ms = 0.f;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!e->gate_pending) return VF_OK;
    HIPCHK(hipEventSynchronize(e->gate_ev[2]));
    if (h2d_ms) HIPCHK(hipEventElapsedTime(h2d_ms, e->gate_ev[0], e->gate_ev[1]));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, e->gate_ev[1], e->gate_ev[2]));
    return VF_OK;
}
