// engine/engine_absolute.inc -- absolute pose and position factors on keyframes, in the between slot (DESIGN.md "4k"): the per-slot
// kind K2 reads (vf_engine::btw_kind; VF_ABSOLUTE_*).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// The array is a late buffer made behind the loss arrays (vf_engine::ensure_kind); the staging calls that write or clear a record
// reset its slot with its loss (vf_engine::reset_loss, engine_staging.inc), vf_engine_compact and vf_engine_grow move it
// (engine_window.inc).  A slide moves no slot, so the kind stays where its factor is.
int vf_absolute_position_record(const double p[3], const double cov9[9], double rec28[28]) {
    if (!p || !cov9 || !rec28) return fail(VF_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(p[i])) return fail(VF_ERR_INVALID, "absolute position: component %d is not finite", i);
    // reverse Cholesky cov = U U^T (U upper), then R3 = U^-1: R3^T R3 = cov^-1, upper triangular
    double U[9] = {0}, T[9] = {0};
    for (int j = 2; j >= 0; j--) {
        double d = cov9[j * 3 + j];
        for (int l = j + 1; l < 3; l++) d -= U[j * 3 + l] * U[j * 3 + l];
        if (!(d > 0.0) || !std::isfinite(d)) return fail(VF_ERR_NOT_SPD, "absolute position: the covariance is not symmetric positive definite");
        const double ujj = std::sqrt(d);
        U[j * 3 + j] = ujj;
        for (int i = 0; i < j; i++) {
            double a = 0.5 * (cov9[i * 3 + j] + cov9[j * 3 + i]);
            for (int l = j + 1; l < 3; l++) a -= U[i * 3 + l] * U[j * 3 + l];
            U[i * 3 + j] = a / ujj;
        }
    }
    for (int c = 0; c < 3; c++) {
        T[c * 3 + c] = 1.0 / U[c * 3 + c];
        for (int r = c - 1; r >= 0; r--) {
            double a = 0.0;
            for (int l = r + 1; l <= c; l++) a += U[r * 3 + l] * T[l * 3 + c];
            T[r * 3 + c] = -a / U[r * 3 + r];
        }
    }
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(T[i])) return fail(VF_ERR_NOT_SPD, "absolute position: the covariance is not symmetric positive definite");
    memset(rec28, 0, 28 * sizeof(double));
    rec28[0] = 1.0;
    for (int i = 0; i < 3; i++) rec28[4 + i] = p[i];
    // the translation block of the 21 packed words: rows 3..5 of the 6 x 6 upper triangle (15..17, 18..19, 20)
    rec28[7 + 15] = T[0]; rec28[7 + 16] = T[1]; rec28[7 + 17] = T[2];
    rec28[7 + 18] = T[4]; rec28[7 + 19] = T[5];
    rec28[7 + 20] = T[8];
    return VF_OK;
}

int vf_engine_set_absolute(vf_engine* e, int window, int n, const int32_t* b, const int32_t* kind, const double* rec28) {
    // (the arguments first, the engine after them: a refused call has touched nothing, the engine stays as warm as it was)
    if (n < 0 || (n > 0 && (!b || !kind || !rec28))) return fail(VF_ERR_INVALID, "null argument");
    for (int i = 0; i < n; i++)
        if (kind[i] != VF_ABSOLUTE_POSE && kind[i] != VF_ABSOLUTE_POSITION)
            return fail(VF_ERR_INVALID, "absolute factor %d: unknown kind %d (a between factor is vf_engine_set_between's)", i, kind[i]);
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (window < 0 || window >= e->v.B) return fail(VF_ERR_INVALID, "window %d out of range", window);
    if (e->v.sh_G > 1) return fail(VF_ERR_INVALID, "vf_engine_set_absolute: losses on time-sharded engines are not built (shard %d of %d)", e->v.sh_r, e->v.sh_G);
    const int M = e->v.M;
    int first = n > 0 ? 1 << 30 : 0;
    for (int i = 0; i < n; i++) {
        if (b[i] - 1 < 0 || b[i] >= M) return fail(VF_ERR_BAD_KEY, "absolute factor %d: need 1 <= b < capacity %d, the factor sits in b's slot as one from b - 1 (b=%d)", i, M, b[i]);
        first = b[i] < first ? b[i] : first;
    }
    Entry entry_(e, Entry::appends(window, first), Entry::overlaps);
    if (n == 0) return VF_OK;
    int rc = e->ensure_kind();
    if (rc) return rc;
    if (e->async_base() && n <= 4) {
        // (record, source and attributes travel as kernel arguments: no staging copy, no synchronisation)
        vf::BtwLossArg la{};
        vf::BtwKindArg ka{};
        la.n = ka.n = n;
        for (int i = 0; i < n; i++) {
            vf::BtwArg arg;
            memcpy(arg.r, rec28 + (size_t)i * vf::BTW_IN, sizeof(arg.r));
            const long g = (long)window * M + b[i];
            vf::launch_put_between(e->v, g, b[i] - 1, arg, e->stream);
            la.g[i] = ka.g[i] = g;
            ka.kind[i] = kind[i];
        }
        vf::launch_put_between_loss(e->v, la, e->stream);       // (a new record is a Gaussian factor until it is given a loss)
        vf::launch_put_between_kind(e->btw_kind, ka, e->stream);
        HIPCHK(hipGetLastError());
        return VF_OK;
    }
    if (e->side_open) { if (int rj = e->join_side()) return rj; }
    // runs of consecutive b in one scatter and one copy per attribute, from host arrays that live until the synchronisation
    std::vector<int> src(n);
    for (int i = 0; i < n; i++) src[i] = b[i] - 1;
    int i = 0;
    while (i < n) {
        int j = i + 1;
        while (j < n && b[j] == b[j - 1] + 1) j++;
        const int cnt = j - i;
        const size_t bytes = (size_t)cnt * vf::BTW_IN * sizeof(double);
        if ((rc = e->ensure_stage(bytes))) return rc;
        HIPCHK(hipMemcpyAsync(e->stage, rec28 + (size_t)i * vf::BTW_IN, bytes, hipMemcpyHostToDevice, e->stream));
        const long g0 = (long)window * M + b[i];
        vf::launch_scatter(e->stage, e->v.btw_in, g0, cnt, vf::BTW_IN, e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(e->v.btw_a + g0, src.data() + i, cnt * sizeof(int), hipMemcpyHostToDevice, e->stream));
        if ((rc = e->reset_loss(g0, cnt))) return rc;
        HIPCHK(hipMemcpyAsync(e->btw_kind + g0, kind + i, cnt * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        i = j;
    }
    return VF_OK;
}

int vf_engine_get_absolute(vf_engine* e, int window, int k0, int n, int32_t* kind) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0 || !kind) return VF_OK;
    if (!e->btw_kind) {
        for (int i = 0; i < n; i++) kind[i] = VF_ABSOLUTE_NONE;
        return VF_OK;
    }
    HIPCHK(hipMemcpyAsync(kind, e->btw_kind + (long)window * e->v.M + k0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}
