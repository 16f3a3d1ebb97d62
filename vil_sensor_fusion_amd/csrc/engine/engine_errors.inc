// engine/engine_errors.inc -- per-factor chi-square errors, a summary per window, the batch's health (vf_engine_factor_errors and
// its readers).  A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C",
// never compiled by itself.
//
// The errors are of the window's current states.  Two ways to the residuals they are made of:
//   reuse        after a solve the current buffer's residuals ARE those of the current states (k_decide's cost[w] is their sum), and
//                SolveMemory knows whether anything has been written since (residuals_vouched).  The call then launches
//                k_factor_errors on what is there and touches nothing else: no event fires, the cached result block stays.
//   relinearise  asked for (VF_ERRORS_RELINEARIZE), or the engine cannot vouch: every factor is linearised at the current states
//                first, every window whether or not the termination rule has finished it (vf::every_window, vf_launch_view.hpp) -- the
//                same bits into the same buffer -- and the engine is marked cold, as after the covariances.
// The result buffer belongs to the call that wrote it: later solves leave it, compact and grow void it (SolveMemory::errors_valid).
int vf_engine_factor_errors(vf_engine* e, unsigned flags, const double* chi2_threshold6) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (flags & ~(unsigned)VF_ERRORS_RELINEARIZE) return fail(VF_ERR_INVALID, "vf_engine_factor_errors: unknown flags 0x%x", flags);
    Entry entry_(e, Entry::reads, Entry::leaves_result);      // (nothing here touches the result block of the last solve)
    if (int rc = not_sharded(e, "vf_engine_factor_errors")) return rc;
    e->mem.excursions = e->excursion() > 0;                   // (as the windows stand now: an engine that refines takes excursions)
    e->recount_far();
    e->mem.errors_started();      // (behind every refusal: a refused call leaves the engine as it was)
    if (!e->err) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->err.ensure(e->err_bytes()));
    }
    if ((flags & VF_ERRORS_RELINEARIZE) || !e->mem.residuals_vouched()) {
        e->mem.rewritten();
        const vf::View a = vf::every_window(e->v);
        vf::launch_linearize(a, e->btw_kind, 0, e->stream);      // (which = 0: the estimate, or theta of a reference-compat engine)
        if (e->x_used > 0) vf::launch_linearize_extra(a, 0, e->stream);     // (launch_linearize leaves the far factors to the caller)
        e->mem.residuals_current();
    }
    vf::FactorErrors o = e->err_view();
    for (int c = 0; c < vf::ERR_CLASSES; c++) {
        const double t = chi2_threshold6 ? chi2_threshold6[c] : 0.0;
        o.thr[c] = std::isfinite(t) && t > 0.0 ? t : INFINITY;
    }
    vf::launch_factor_errors(e->v, o, e->stream);
    HIPCHK(hipGetLastError());
    e->err_lo = e->h_lo;
    e->err_hi = e->h_hi;
    e->mem.errors_computed();
    return VF_OK;
}

// What every reader refuses, in this order: a window that is not there; results that are not.  Then the one synchronisation of a read.
static int check_errors(vf_engine* e, int window, const char* what) {
    if (int rc = check_window(e, window)) return rc;
    if (!e->mem.errors_valid())
        return fail(VF_ERR_INVALID, "%s: no factor errors: call vf_engine_factor_errors first (vf_engine_compact and vf_engine_grow void them)", what);
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}
// an output struct the caller sized: the library's bytes as far as the caller's struct goes
// (struct_size is the first word of both output structs; `full`: the library's size of the one at hand)
static int put_sized(void* out, size_t full, const void* dev, const char* what) {
    if (!out) return fail(VF_ERR_INVALID, "%s: null output", what);
    uint32_t n;
    memcpy(&n, out, sizeof(n));
    if (n < sizeof(uint32_t) || n > full)
        return fail(VF_ERR_INVALID, "%s: struct_size = %u: this library knows sizes up to %zu (fill it with sizeof)", what, n, full);
    unsigned char buf[sizeof(vf_consistency)];
    static_assert(sizeof(vf_batch_health) <= sizeof(vf_consistency), "the larger of the two output structs");
    HIPCHK(hipMemcpy(buf, dev, full, hipMemcpyDeviceToHost));
    memcpy(buf, &n, sizeof(n));
    memcpy(out, buf, n);
    return VF_OK;
}

int vf_engine_read_factor_errors(vf_engine* e, int window, int k0, int n, double* imu_err, double* btw_err, int32_t* btw_a) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_errors(e, window, "vf_engine_read_factor_errors")) return rc;
    if (n < 0 || k0 < e->err_lo[window] || k0 + n > e->err_hi[window])
        return fail(VF_ERR_BAD_KEY, "vf_engine_read_factor_errors: keyframes [%d,%d) outside the range [%d,%d) the errors were computed for", k0, k0 + n,
                    e->err_lo[window], e->err_hi[window]);
    if (n == 0) return VF_OK;
    const vf::FactorErrors o = e->err_view();
    const size_t g = (size_t)window * e->v.M + k0;
    std::vector<double> eb((size_t)n);
    HIPCHK(hipMemcpy(eb.data(), o.btw + g, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (imu_err) HIPCHK(hipMemcpy(imu_err, o.imu + g, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (btw_err) memcpy(btw_err, eb.data(), (size_t)n * sizeof(double));
    if (btw_a) {
        // (the engine's own list: the slot a factor starts from, where the call found one alive)
        HIPCHK(hipMemcpy(btw_a, e->v.btw_a + g, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++)
            if (eb[i] == -1.0) btw_a[i] = -1;
    }
    return VF_OK;
}

int vf_engine_read_far_errors(vf_engine* e, int window, double* far_err, double* far_linear_err) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_errors(e, window, "vf_engine_read_far_errors")) return rc;
    const vf::FactorErrors o = e->err_view();
    const double* src = o.far + (size_t)window * 2 * o.x_cap;
    if (far_err) HIPCHK(hipMemcpy(far_err, src, (size_t)o.x_cap * sizeof(double), hipMemcpyDeviceToHost));
    if (far_linear_err) HIPCHK(hipMemcpy(far_linear_err, src + o.x_cap, (size_t)o.x_cap * sizeof(double), hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_engine_read_consistency(vf_engine* e, int window, vf_consistency* out) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_errors(e, window, "vf_engine_read_consistency")) return rc;
    return put_sized(out, sizeof(vf_consistency), e->err_view().summary + window, "vf_engine_read_consistency");
}

int vf_engine_read_health(vf_engine* e, vf_batch_health* out) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_errors(e, 0, "vf_engine_read_health")) return rc;
    return put_sized(out, sizeof(vf_batch_health), e->err_view().health, "vf_engine_read_health");
}
