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
    const int B = e->v.B;
    if (int rc = check_tail_steps(e, "vf_engine_gate_tail", step_off, steps,
                                  "needs the marginal covariances of the last keyframes: call vf_engine_marginals_ex first (VF_MARGINALS_TAIL is enough)")) return rc;
    // one packed block: [offsets B + 1][btw_a B][first slot the covariances cover B] | [records 28 x B][steps 7 x total]
    vf::Packed blk;
    const size_t rec_b = (size_t)B * vf::BTW_IN * sizeof(double), st_b = (size_t)step_off[B] * 7 * sizeof(double);
    const size_t int_at = blk.add((size_t)(3 * B + 1) * sizeof(int)), rec_at = blk.add(rec_b), st_at = blk.add(st_b);
    if (!e->gate_out) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->gate_out.ensure((size_t)B * vf::GATE_RECORD));
    }
    char* h = nullptr;
    HIPCHK(e->gate.open(blk.bytes, &h));
    int* hi32 = (int*)(h + int_at);
    memcpy(hi32, step_off, (size_t)(B + 1) * sizeof(int));
    memcpy(hi32 + B + 1, btw_a, (size_t)B * sizeof(int));
    memcpy(hi32 + 2 * B + 1, e->sig_lo.data(), (size_t)B * sizeof(int));
    memcpy(h + rec_at, btw_rec28, rec_b);
    if (st_b > 0) memcpy(h + st_at, steps, st_b);
    HIPCHK(e->gate.send(blk.bytes, e->stream, true));
    const char* d = e->gate.device();
    const int* d32 = (const int*)(d + int_at);
    const double thr = std::isfinite(chi2_threshold) && chi2_threshold > 0.0 ? chi2_threshold : INFINITY;
    vf::launch_gate_between(e->v, d32, (const double*)(d + st_at), imu_cov(p), d32 + B + 1, d32 + 2 * B + 1, (const double*)(d + rec_at), thr,
                            (flags & VF_GATE_FROM_ESTIMATE) ? 1 : 0, e->sig, e->sig_fail(), e->gate_out.get(), e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(e->gate.launched(e->stream));
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
    HIPCHK(e->gate.timings(h2d_ms, kernel_ms));
    return VF_OK;
}
