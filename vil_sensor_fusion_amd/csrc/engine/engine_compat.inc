// engine/engine_compat.inc -- the reference-compat update (one iSAM2-like Gauss-Newton update) and its incremental form.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// ------------------------------------------------------------------ reference-compat solve
// What the reference does per GraphManager::solve (GraphManager.cpp:38-43,126-127): ONE iSAM2 update -- Gauss-Newton
// (QR, no damping) about per-variable linearisation points theta, relinearising only the variables whose pending
// increment reaches relinearizeThreshold (1e-4) -- and calculateEstimate() = theta (+) delta.  Here: buffer sel = theta,
// v.delta = delta, the trial buffer = the estimate.  iSAM2 re-eliminates only the cliques a new factor touches; solving the
// whole banded system with every factor linearised at theta gives the same increment (its partial back-substitution
// stops below wildfireThreshold 1e-3 * ... of change; that approximation is NOT reproduced -- the full solve is exact).
// the opening of such an update, also for time-sharded engines (the caller then runs the staged solve -- vf_engine_assemble,
// vf_engine_solve_local, ..., the refinement -- and vf_engine_retract): relinearise where the pending increment reaches the
// threshold, lambda := 0 (Gauss-Newton), linearise every factor at theta
int vf_engine_gn_begin(vf_engine* e, double relin_threshold) {
    VF_ENTER(e, Entry::reads);
    if (!(relin_threshold >= 0.0)) return fail(VF_ERR_INVALID, "relinearisation threshold must be >= 0");
    e->mem.rewritten();
    int rc;
    vf::launch_relinearize(e->v, relin_threshold, e->stream);
    HIPCHK(hipMemsetAsync(e->v.lambda, 0, e->v.B * sizeof(double), e->stream));     // Gauss-Newton: no damping
    if ((rc = vf_engine_linearize(e, 0)) || (rc = vf_engine_decide(e, 1))) return rc;
    return VF_OK;
}
// The same update done incrementally (vf_engine_opts.incremental): relinearise, then linearise / assemble / eliminate only from
// the first keyframe that changed, back-substitute until the increments stop changing (vf_kernels.hpp "Incremental
// Gauss-Newton updates").  The first update of an engine, and every update after an entry point the bookkeeping does not
// follow, covers the whole window.
// the failure flags of the solve just enqueued, read back: the first window that failed is the one reported
static int first_failed_window(vf_engine* e) {
    std::vector<int> failed((size_t)e->v.B);
    HIPCHK(hipMemcpyAsync(failed.data(), e->v.fail, failed.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int w = 0; w < e->v.B; w++)
        if (failed[w]) return fail(VF_ERR_INDETERMINATE, "window %d: normal equations not positive definite (underdetermined graph)", w);
    return VF_OK;
}
static int isam_step_incremental(vf_engine* e, double relin_threshold) {
    const int invalid = (e->mem.inc_whole_window() || e->opts.incremental == 2) ? 1 : 0;     // (incremental = 2: the same kernels over the whole window, every time)
    const int appended = e->mem.inc_appended(e->h_hi[0]);
    const vf::View a = vf::incremental(e->v, invalid || e->mem.inc_slid());     // (the priors too where the marginal prior has changed)
    vf::launch_inc_begin(a, relin_threshold, appended, invalid, e->stream);
    HIPCHK(hipMemsetAsync(e->v.lambda, 0, e->v.B * sizeof(double), e->stream));     // Gauss-Newton: no damping
    vf::launch_linearize(a, e->btw_kind, 0, e->stream);
    vf::launch_assemble(a, e->stream);
    vf::launch_inc_solve(a, e->stream);
    vf::launch_inc_retract(a, e->stream);
    HIPCHK(hipGetLastError());
    e->inc_updates++;
    if (invalid) e->inc_full++;
    const int rc = first_failed_window(e);
    e->mem.inc_update_ended(rc == VF_OK);
    return rc;
}
int vf_engine_isam_step(vf_engine* e, double relin_threshold) {
    VF_ENTER(e, Entry::reads);
    if (int rc0 = not_sharded(e, "vf_engine_isam_step")) return rc0;
    if (!(relin_threshold >= 0.0)) return fail(VF_ERR_INVALID, "relinearisation threshold must be >= 0");
    // (far factors are solved as a low-rank correction of the whole band: such windows take the full update)
    if (e->v.ck && e->x_used == 0 && e->refine_iters() == 0) return isam_step_incremental(e, relin_threshold);
    int rc;
    if ((rc = vf_engine_gn_begin(e, relin_threshold)) || (rc = vf_engine_assemble(e)) ||
        (rc = vf_engine_solve(e)) || (rc = vf_engine_retract(e))) return rc;
    if ((rc = first_failed_window(e))) return rc;
    e->mem.rewritten();
    e->mem.residuals_current();     // (linearised at theta by vf_engine_gn_begin; the solve and the retraction wrote the trial buffer)
    return VF_OK;
}
int vf_engine_incremental_info(vf_engine* e, int window, long* updates, long* whole_window_updates, int* first_eliminated, int* last_substituted) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    if (updates) *updates = e->inc_updates;
    if (whole_window_updates) *whole_window_updates = e->inc_full;
    int from = -1, stop = -1;
    if (e->v.ck) {
        HIPCHK(hipMemcpyAsync(&from, e->v.inc_from + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&stop, e->v.inc_stop + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (first_eliminated) *first_eliminated = from;
    if (last_substituted) *last_substituted = stop;
    return VF_OK;
}
int vf_engine_predict_from_estimate(vf_engine* e, int window, int k0, int n) {
    VF_ENTER(e, Entry::reads, Entry::overlaps_if(e && window >= 0 && window < e->v.B && k0 > e->h_lo[window] + 1));
    e->mem.predicted_from_estimate(window, k0, e->h_lo[0]);
    if (window >= e->v.B || k0 < 1 || n < 0 || k0 + n > e->v.M) return fail(VF_ERR_BAD_KEY, "bad predict range");
    if (n == 0) return VF_OK;
    vf::launch_predict(e->v, window, k0, n, 1, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
int vf_engine_get_estimate(vf_engine* e, int window, int k0, int n, double* s) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (!s) return fail(VF_ERR_INVALID, "null states");
    if (n == 0) return VF_OK;
    const size_t bytes = (size_t)n * 16 * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    vf::launch_gather_states(e->v.x, e->stage, e->v.G, e->v.sel, e->v.M, 1, (long)window * e->v.M + k0, n, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s, e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}
