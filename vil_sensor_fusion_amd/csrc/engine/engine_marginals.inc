// engine/engine_marginals.inc -- marginal covariances of the solved keyframes (vf_engine_marginals / vf_engine_read_marginals).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.
//
// The undamped factorisation at the current states is made on a COPY of the View whose lambda, failure flags and `fresh` flags
// point at arrays of this section: the LM state of the engine (states, increments, lambda, counters, done flags, sticky words,
// the cached result block) is not touched.  What is overwritten -- the current buffer's linearisation (the same bits: it is of
// the same states), H, g and the panels -- is what a cold start rebuilds, and the engine is marked cold.
int vf_engine_marginals(vf_engine* e) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    const bool cached = e->res_cached;
    DeviceGuard dev_guard_(e);
    e->res_cached = cached;      // (nothing here touches the result block of the last solve)
    if (int rc = not_sharded(e, "vf_engine_marginals")) return rc;
    e->recount_far();
    if (e->x_used > 0)
        return fail(VF_ERR_INVALID, "vf_engine_marginals: a window holds far factors (vf_engine_get_extra_between / vf_engine_get_linear_far); "
                    "their correction of the covariance is not implemented");
    const size_t G = (size_t)e->v.G, B = (size_t)e->v.B;
    if (!e->sig || e->sig_G != e->v.G) {
        // allocated on first use (G x 2.7 KB): engines that never ask for covariances do not grow
        if (e->sig) { HIPCHK(hipStreamSynchronize(e->stream)); (void)hipFree(e->sig); e->sig = nullptr; }
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, G * vf::SIG_SLOT * sizeof(double) + B * (sizeof(double) + 2 * sizeof(int)) + 256));
        e->sig = (double*)q;
        e->sig_G = e->v.G;
        e->sig_zero = e->sig + G * vf::SIG_SLOT;
        e->sig_fail = (int*)(e->sig_zero + B);
        e->sig_ones = e->sig_fail + B;
        std::vector<int> ones(B, 1);
        HIPCHK(hipMemsetAsync(e->sig_zero, 0, B * sizeof(double), e->stream));
        HIPCHK(hipMemcpyAsync(e->sig_ones, ones.data(), B * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    cold(e);
    vf::View a = e->v;
    a.lambda = e->sig_zero;          // undamped
    a.fail = e->sig_fail;
    a.fresh = e->sig_ones;           // every window assembled, whole
    a.stop_on = 0;                   // ... whether or not the termination rule has finished it
    a.gate = 0;
    a.act = nullptr;
    a.inc_on = 0;
    a.relin_only = 0;
    a.P = 0;                         // whole-window sweep whatever form the engine's solves take (they may be partitioned)
    HIPCHK(hipMemsetAsync(e->sig_fail, 0, B * sizeof(int), e->stream));
    // linearisation at the current states (which = 0): the estimate, or theta of a reference-compat engine
    vf::launch_linearize(a, 0, e->stream);
    // the forward sweep of the engine's own solves when they assemble H themselves (form 2), else k_band_forward after K3
    const vf::SolvePlan plan = solve_plan(e);
    if (plan.factor == vf::Sweep::split) vf::launch_assemble(a, e->stream);
    vf::launch_band_factor(a, plan, e->stream);
    vf::launch_selinv(a, e->sig_fail, e->sig, e->stream);
    HIPCHK(hipGetLastError());
    e->sig_lo = e->h_lo;
    e->sig_hi = e->h_hi;
    e->sig_valid = true;
    return VF_OK;
}

int vf_engine_read_marginals(vf_engine* e, int window, int k0, int n, double* cov225, double* cross225) {
    DeviceGuard dev_guard_(e);
    int rc = check_window(e, window);
    if (rc) return rc;
    if (!e->sig_valid || e->sig_G != e->v.G) return fail(VF_ERR_INVALID, "no marginal covariances: call vf_engine_marginals first");
    if (n < 0 || k0 < e->sig_lo[window] || k0 + n > e->sig_hi[window])
        return fail(VF_ERR_BAD_KEY, "keyframes [%d,%d) outside the range [%d,%d) the covariances were computed for", k0, k0 + n,
                    e->sig_lo[window], e->sig_hi[window]);
    int failed = 0;
    HIPCHK(hipMemcpyAsync(&failed, e->sig_fail + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (failed) return fail(VF_ERR_NOT_SPD, "window %d: the undamped normal equations are not positive definite", window);
    if (n == 0 || (!cov225 && !cross225)) return VF_OK;
    std::vector<double> raw((size_t)n * vf::SIG_SLOT);
    HIPCHK(hipMemcpy(raw.data(), e->sig + ((size_t)window * e->v.M + k0) * vf::SIG_SLOT, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) {
        const double* r = raw.data() + (size_t)k * vf::SIG_SLOT;
        if (cov225)
            for (int a = 0; a < 15; a++)
                for (int c = 0; c < 15; c++) cov225[(size_t)k * 225 + a * 15 + c] = r[a >= c ? vf::h_tri(a, c) : vf::h_tri(c, a)];
        if (cross225) memcpy(cross225 + (size_t)k * 225, r + 120, 225 * sizeof(double));
    }
    return VF_OK;
}
