// engine/engine_misc.inc -- termination rule, damping reset, prediction.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
int vf_engine_set_convergence(vf_engine* e, double rel_tol, double abs_tol) {
    VF_ENTER(e, Entry::rewrites);
    if (!(rel_tol >= 0.0) || !(abs_tol >= 0.0)) return fail(VF_ERR_INVALID, "tolerances must be >= 0");
    HIPCHK(hipStreamSynchronize(e->stream));
    e->v.rel_tol = rel_tol;
    e->v.abs_tol = abs_tol;
    e->v.stop_on = (rel_tol > 0.0 || abs_tol > 0.0) ? 1 : 0;
    e->epoch++;
    // sweep engines (large batches): once few windows are left taking trials, K4 switches to the partitioned form
    if (e->v.stop_on && e->v.P == 0 && e->v.B > 128 && !e->hybrid && e->tune.hybrid_threshold >= 0) {
        vf::View& v = e->v;
        e->hybrid_P = vf::chunk_count(v.M, 96, 1);
        if (e->hybrid_P >= 2) {
            const size_t BP = (size_t)v.B * e->hybrid_P;
            int rc;
            if ((rc = e->alloc(&e->h_Vp, (size_t)v.G * vf::VROW)) || (rc = e->alloc(&e->h_sep, BP * vf::SEPK)) ||
                (rc = e->alloc(&e->h_sepL, BP * vf::SEPL)) || (e->tune.hybrid_active_list && (rc = e->alloc(&e->act_list, (size_t)v.B)))) return rc;
            e->hybrid = true;
        }
    }
    HIPCHK(hipMemsetAsync(e->v.done, 0, e->v.B * sizeof(int), e->stream));
    return VF_OK;
}
int vf_engine_reset_lambda(vf_engine* e) {
    VF_ENTER(e, Entry::reads);
    vf::launch_reset_lambda(e->v, e->lambda0_dev, 0, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}

int vf_engine_predict(vf_engine* e, int window, int k0, int n) {
    // (inherited order: the write is recorded before the range is validated)
    VF_ENTER(e, Entry::appends(window, k0), Entry::overlaps_if(e && window >= 0 && window < e->v.B && k0 > e->h_lo[window] + 1));
    if (window >= e->v.B || k0 < 1 || n < 0 || k0 + n > e->v.M) return fail(VF_ERR_BAD_KEY, "bad predict range");
    if (n == 0) return VF_OK;
    vf::launch_predict(e->v, window, k0, n, 0, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
