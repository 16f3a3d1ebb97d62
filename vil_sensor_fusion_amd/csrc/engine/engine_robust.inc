// engine/engine_robust.inc -- robust losses of the band between factors: the per-slot attribute K2 reads (View::btw_loss, btw_loss_k).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// The arrays are late buffers (vf_engine::ensure_loss); the staging calls that write or clear a record reset its slot
// (vf_engine::reset_loss, engine_staging.inc), vf_engine_compact and vf_engine_grow move them (engine_window.inc).
int vf_engine_set_between_loss(vf_engine* e, int window, int n, const int32_t* b, const int32_t* loss, const double* k) {
    int first = n > 0 ? 1 << 30 : 0;
    for (int i = 0; i < n && b; i++) first = b[i] < first ? b[i] : first;
    // (the arguments first, the engine after them: a refused call has touched nothing, the engine stays as warm as it was)
    if (n < 0 || (n > 0 && (!b || !loss || !k))) return fail(VF_ERR_INVALID, "null argument");
    bool any = false;
    for (int i = 0; i < n; i++) {
        if (loss[i] < VF_LOSS_NONE || loss[i] > VF_LOSS_GEMAN_MCCLURE) return fail(VF_ERR_INVALID, "between loss %d: unknown loss id %d", i, loss[i]);
        if (loss[i] != VF_LOSS_NONE && !(k[i] > 0.0 && std::isfinite(k[i]))) return fail(VF_ERR_INVALID, "between loss %d: the parameter k must be finite and > 0 (got %g)", i, k[i]);
        any = any || loss[i] != VF_LOSS_NONE;
    }
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    Entry entry_(e, Entry::appends(window, first), Entry::overlaps);
    int rc = check_window(e, window);
    if (rc) return rc;
    if (e->v.sh_G > 1) return fail(VF_ERR_INVALID, "vf_engine_set_between_loss: losses on time-sharded engines are not built (shard %d of %d)", e->v.sh_r, e->v.sh_G);
    const int M = e->v.M;
    for (int i = 0; i < n; i++)
        if (b[i] < 0 || b[i] >= M) return fail(VF_ERR_BAD_KEY, "between loss %d: slot %d outside capacity %d", i, b[i], M);
    if (n == 0 || (!any && !e->v.btw_loss)) return VF_OK;       // (NONE on an engine without the arrays: what it holds already)
    if ((rc = e->ensure_loss())) return rc;
    if (e->async_base() && n <= 4) {
        // (the attributes travel as a kernel argument: no staging copy, no synchronisation)
        vf::BtwLossArg la{};
        la.n = n;
        for (int i = 0; i < n; i++) {
            la.g[i] = (long)window * M + b[i];
            la.loss[i] = loss[i];
            la.k[i] = loss[i] == VF_LOSS_NONE ? 0.0 : k[i];
        }
        vf::launch_put_between_loss(e->v, la, e->stream);
        HIPCHK(hipGetLastError());
        return VF_OK;
    }
    if (e->side_open) { if (int rj = e->join_side()) return rj; }
    // runs of consecutive slots in one copy each, from host arrays that live until the synchronisation below
    std::vector<double> kk(k, k + n);
    for (int i = 0; i < n; i++) if (loss[i] == VF_LOSS_NONE) kk[i] = 0.0;
    int i = 0;
    while (i < n) {
        int j = i + 1;
        while (j < n && b[j] == b[j - 1] + 1) j++;
        const long g0 = (long)window * M + b[i];
        HIPCHK(hipMemcpyAsync(e->v.btw_loss + g0, loss + i, (size_t)(j - i) * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->v.btw_loss_k + g0, kk.data() + i, (size_t)(j - i) * sizeof(double), hipMemcpyHostToDevice, e->stream));
        i = j;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_get_between_loss(vf_engine* e, int window, int k0, int n, int32_t* loss, double* k) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0) return VF_OK;
    if (!e->v.btw_loss) {
        for (int i = 0; i < n; i++) { if (loss) loss[i] = VF_LOSS_NONE; if (k) k[i] = 0.0; }
        return VF_OK;
    }
    const long g0 = (long)window * e->v.M + k0;
    if (loss) HIPCHK(hipMemcpyAsync(loss, e->v.btw_loss + g0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if (k) HIPCHK(hipMemcpyAsync(k, e->v.btw_loss_k + g0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

// ---- robust losses of the far between factors: an attribute of the list ENTRY (vf_engine::h_xloss, h_xk; on the device behind the
// records of View::x_in, vf::far_loss).  The list is replaced as a whole, so the losses come with it (set_far_list, engine_staging.inc).
int vf_engine_set_extra_between_robust(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec28,
                                       const int32_t* loss, const double* k) {
    // (the arguments first, the engine after them: a refused call has touched nothing)
    if (n > 0 && (!loss || !k)) return fail(VF_ERR_INVALID, "null argument");
    for (int i = 0; i < n; i++) {
        if (loss[i] < VF_LOSS_NONE || loss[i] > VF_LOSS_GEMAN_MCCLURE) return fail(VF_ERR_INVALID, "far between loss %d: unknown loss id %d", i, loss[i]);
        if (loss[i] != VF_LOSS_NONE && !(k[i] > 0.0 && std::isfinite(k[i]))) return fail(VF_ERR_INVALID, "far between loss %d: the parameter k must be finite and > 0 (got %g)", i, k[i]);
    }
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (e->v.sh_G > 1) return fail(VF_ERR_INVALID, "vf_engine_set_extra_between_robust: losses on time-sharded engines are not built (shard %d of %d)", e->v.sh_r, e->v.sh_G);
    return set_far_list(e, window, n, a, b, rec28, loss, k);
}

int vf_engine_get_extra_between_loss(vf_engine* e, int window, int32_t* loss, double* k) {
    int rc = check_window(e, window);
    if (rc) return rc;
    const int cnt = e->v.x_max ? e->h_xn[window] : 0;
    for (int i = 0; i < e->x_cap; i++) {
        if (loss) loss[i] = i < cnt ? e->h_xloss[window][i] : VF_LOSS_NONE;
        if (k) k[i] = i < cnt ? e->h_xk[window][i] : 0.0;
    }
    return VF_OK;
}

int vf_engine_read_extra_lin(vf_engine* e, int window, int which, double* r6, double* Ja, double* Jb) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    const int X = e->x_cap;
    std::vector<double> h((size_t)X * vf::BTW_OUT, 0.0);
    if (e->v.x_max > 0) {
        int sel = 0;
        if ((rc = read_sel(e, window, &sel))) return rc;
        const int b = sel ^ (which ? 1 : 0);
        HIPCHK(hipMemcpyAsync(h.data(), e->v.x_out + ((size_t)b * e->v.B + window) * X * vf::BTW_OUT, h.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    for (int i = 0; i < X; i++) {
        const double* p = h.data() + (size_t)i * vf::BTW_OUT;
        if (r6) memcpy(r6 + (size_t)i * 6, p, 6 * sizeof(double));
        if (Ja) memcpy(Ja + (size_t)i * 36, p + 6, 36 * sizeof(double));
        if (Jb) memcpy(Jb + (size_t)i * 36, p + 42, 36 * sizeof(double));
    }
    return VF_OK;
}
