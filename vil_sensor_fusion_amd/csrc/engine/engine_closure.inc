// engine/engine_closure.inc -- the loop-closure gate: chi-square of a candidate between factor on any two solved keyframes of a
// window, before it is added (vf_engine_gate_closures / vf_engine_read_closure_gate / vf_engine_read_closure_gate_all /
// vf_engine_closure_gate_status; kernels/kclosure.inc; DESIGN.md section 4j).  A section of vf_engine.hip (the C ABI of the engine:
// include/vilfusion.h); included from there behind engine_marginals.inc, inside extern "C", never compiled by itself.
//
// The call makes the undamped factorisation itself (factor_undamped, engine_marginals.inc: what vf_engine_marginals_ex starts
// with), then per group of windows the unit columns of the candidates' keyframes, Z and R of the far factors alive, and the gate
// kernel.  What it overwrites is what that half of vf_engine_marginals_ex overwrites -- the current buffer's linearisation (same
// bits), H, g, the panels: the engine is left cold -- and buffers of its own.  sig, its flags and its validity, states, the LM
// state, the result block, errors, the propagation and the tail gate's result are as they were.
//
// Scratch, per window of a group: M x 15 x 6 K doubles of unit columns (K: the most distinct candidate keyframes a window of the
// call has, 8 at most) and, with far factors alive, FarCov's Z and C.  Groups are budgeted as the marginals' (FARCOV_BUDGET), over
// the span of windows that hold a candidate.
static_assert(sizeof(vf_closure_gate_result) == vf::CLOSURE_RECORD, "vf_closure_gate_result and its device twin (kernels/kclosure.inc)");
static_assert(VF_CLOSURE_GATE_MAX == vf::CLOSURE_MAX, "VF_CLOSURE_GATE_MAX and its device twin");
int vf_engine_gate_closures(vf_engine* e, int n, const int32_t* window, const int32_t* a, const int32_t* b, const double* rec28,
                            double chi2_threshold) {
    return vf_engine_gate_closures_ex(e, n, window, a, b, rec28, chi2_threshold, 0u);
}
int vf_engine_gate_closures_ex(vf_engine* e, int n, const int32_t* window, const int32_t* a, const int32_t* b, const double* rec28,
                               double chi2_threshold, unsigned flags) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (flags & ~(unsigned)VF_GATE_FROM_ESTIMATE) return fail(VF_ERR_INVALID, "vf_engine_gate_closures_ex: unknown flags 0x%x", flags);
    if (n < 0 || (n > 0 && (!window || !a || !b || !rec28))) return fail(VF_ERR_INVALID, "vf_engine_gate_closures: null argument or n < 0");
    if (int rc = not_sharded(e, "vf_engine_gate_closures")) return rc;
    const int B = e->v.B;
    // per window: which candidates, and the distinct keyframes of those that can be tested (ascending)
    std::vector<int> cnt((size_t)B, 0), idx((size_t)B * vf::CLOSURE_MAX, 0), nkeys((size_t)B, 0), keys((size_t)B * vf::CLOSURE_KEYS, -1), status((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const int w = window[i];
        if (w < 0 || w >= B) return fail(VF_ERR_BAD_KEY, "vf_engine_gate_closures: candidate %d: window %d does not exist", i, w);
        if (cnt[w] == vf::CLOSURE_MAX)
            return fail(VF_ERR_CAPACITY, "vf_engine_gate_closures: more than %d candidates on window %d", vf::CLOSURE_MAX, w);
        idx[(size_t)w * vf::CLOSURE_MAX + cnt[w]++] = i;
        status[i] = a[i] == -1 ? VF_GATE_NONE : (a[i] >= b[i] || a[i] < e->h_lo[w] || b[i] >= e->h_hi[w] ? VF_GATE_OUT_OF_REACH : VF_GATE_OK);
    }
    int kmax = 0, wmin = B, wmax = -1;
    for (int i = 0; i < n; i++) {
        if (status[i] != VF_GATE_OK) continue;
        const int w = window[i];
        int* k = keys.data() + (size_t)w * vf::CLOSURE_KEYS;
        for (int key : {a[i], b[i]})
            if (std::find(k, k + nkeys[w], key) == k + nkeys[w]) k[nkeys[w]++] = key;
        std::sort(k, k + nkeys[w]);
        kmax = std::max(kmax, nkeys[w]);
    }
    for (int w = 0; w < B; w++)
        if (cnt[w] > 0) wmin = std::min(wmin, w), wmax = std::max(wmax, w);
    e->recount_far();
    e->mem.closure_gated(0);           // (behind every refusal: a refused call leaves the last result readable)
    if (n == 0) return VF_OK;
    const int m = kmax > 0 ? 6 * e->x_used : 0, nc = 6 * kmax, span = wmax - wmin + 1;
    const size_t xwin = (size_t)e->v.M * 15 * nc, zwin = (size_t)e->v.M * 15 * m, cwin = (size_t)m * m;
    const size_t per = std::max<size_t>(1, xwin + zwin + cwin) * sizeof(double);
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)span, FARCOV_BUDGET / per));
    const size_t out_bytes = (size_t)n * (vf::CLOSURE_RECORD + 144 * sizeof(double));
    if ((size_t)group * per > e->cg_scratch.bytes() || out_bytes > e->cg_out.bytes() || !e->cg_aux) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->cg_scratch.ensure((size_t)group * per));
        HIPCHK(e->cg_out.ensure(out_bytes));
        if (!e->cg_aux) {
            HIPCHK(e->cg_aux.ensure((size_t)B * (sizeof(double) + 2 * sizeof(int)) + 8));
            std::vector<int> ones((size_t)B, 1);
            HIPCHK(hipMemsetAsync(e->cg_zero(), 0, (size_t)B * sizeof(double), e->stream));
            HIPCHK(hipMemcpyAsync(e->cg_ones(), ones.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
        }
    }
    // one packed block: [cnt B][idx 4 B][nkeys B][keys 8 B][a n][b n][status n] | [records 28 x n]
    vf::Packed blk;
    const size_t nB = (size_t)B, int_at = blk.add((nB * (2 + vf::CLOSURE_MAX + vf::CLOSURE_KEYS) + 3 * (size_t)n) * sizeof(int));
    const size_t rec_b = (size_t)n * vf::BTW_IN * sizeof(double), rec_at = blk.add(rec_b);
    char* h = nullptr;
    HIPCHK(e->closure.open(blk.bytes, &h));
    int* hi32 = (int*)(h + int_at);
    const size_t o_cnt = 0, o_idx = nB, o_nk = o_idx + nB * vf::CLOSURE_MAX, o_keys = o_nk + nB, o_a = o_keys + nB * vf::CLOSURE_KEYS, o_b = o_a + n, o_st = o_b + n;
    memcpy(hi32 + o_cnt, cnt.data(), nB * sizeof(int));
    memcpy(hi32 + o_idx, idx.data(), idx.size() * sizeof(int));
    memcpy(hi32 + o_nk, nkeys.data(), nB * sizeof(int));
    memcpy(hi32 + o_keys, keys.data(), keys.size() * sizeof(int));
    memcpy(hi32 + o_a, a, (size_t)n * sizeof(int));
    memcpy(hi32 + o_b, b, (size_t)n * sizeof(int));
    memcpy(hi32 + o_st, status.data(), (size_t)n * sizeof(int));
    memcpy(h + rec_at, rec28, rec_b);
    HIPCHK(e->closure.send(blk.bytes, e->stream, true));
    const int* d32 = (const int*)(e->closure.device() + int_at);
    // no candidate can be tested (every one NONE or OUT_OF_REACH): the kernel writes the records the host already knows, nothing is
    // factored and the engine stays as warm as it was
    vf::View av = e->v;
    if (kmax > 0) {
        if (int rc = factor_undamped(e, e->cg_zero(), e->cg_fail(), e->cg_ones(), &av)) return rc;
    } else HIPCHK(hipMemsetAsync(e->cg_fail(), 0, (size_t)B * sizeof(int), e->stream));
    vf::ClosureGate cg{};
    cg.X = e->cg_scratch;
    cg.keys = d32 + o_keys; cg.nkeys = d32 + o_nk; cg.cnt = d32 + o_cnt; cg.idx = d32 + o_idx;
    cg.a = d32 + o_a; cg.b = d32 + o_b; cg.status = d32 + o_st;
    cg.rec = (const double*)(e->closure.device() + rec_at);
    cg.failed = e->cg_fail();
    cg.out = e->cg_out;
    cg.joint = (double*)(e->cg_out.get() + (((size_t)n * vf::CLOSURE_RECORD + 7) & ~(size_t)7));
    cg.threshold = std::isfinite(chi2_threshold) && chi2_threshold > 0.0 ? chi2_threshold : INFINITY;
    cg.xwin = xwin;
    cg.nc = nc;
    cg.from_estimate = (flags & VF_GATE_FROM_ESTIMATE) ? 1 : 0;
    vf::FarCov fc{};
    fc.Z = e->cg_scratch + (size_t)group * xwin;
    fc.C = fc.Z + (size_t)group * zwin;
    fc.failed = e->cg_fail();
    fc.m = m;
    fc.slots = e->x_used;
    fc.zwin = zwin;
    fc.cwin = cwin;
    for (int w0 = wmin; w0 <= wmax; w0 += group) {
        const int nw = std::min(group, wmax + 1 - w0);
        if (std::all_of(cnt.begin() + w0, cnt.begin() + w0 + nw, [](int c) { return c == 0; })) continue;
        cg.w0 = fc.w0 = w0;
        vf::launch_closure_gate(av, cg, fc, nw, e->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(e->closure.launched(e->stream));
    if (kmax > 0) e->mem.residuals_current();
    e->mem.closure_gated(n);
    return VF_OK;
}

static int check_closure_gate(vf_engine* e, int index, const char* what) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (e->mem.closure_gate_count() == 0)
        return fail(VF_ERR_INVALID, "%s: no result: call vf_engine_gate_closures first (vf_engine_compact and vf_engine_grow void it)", what);
    if (index < 0 || index >= e->mem.closure_gate_count())
        return fail(VF_ERR_BAD_KEY, "%s: candidate %d: the last vf_engine_gate_closures held %d", what, index, e->mem.closure_gate_count());
    return VF_OK;
}

int vf_engine_read_closure_gate(vf_engine* e, int index, vf_closure_gate_result* out, double* joint_cov144) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (int rc = check_closure_gate(e, index, "vf_engine_read_closure_gate")) return rc;
    if (!out) return fail(VF_ERR_INVALID, "vf_engine_read_closure_gate: null output");
    const uint32_t sz = out->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(vf_closure_gate_result))
        return fail(VF_ERR_INVALID, "vf_engine_read_closure_gate: struct_size = %u: this library knows sizes up to %zu (fill it with sizeof)", sz,
                    sizeof(vf_closure_gate_result));
    const size_t n = (size_t)e->mem.closure_gate_count();
    vf_closure_gate_result r;
    HIPCHK(hipMemcpyAsync(&r, e->cg_out.get() + (size_t)index * vf::CLOSURE_RECORD, sizeof(r), hipMemcpyDeviceToHost, e->stream));
    if (joint_cov144)
        HIPCHK(hipMemcpyAsync(joint_cov144, e->cg_out.get() + ((n * vf::CLOSURE_RECORD + 7) & ~(size_t)7) + (size_t)index * 144 * sizeof(double),
                              144 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    r.struct_size = sz;
    memcpy(out, &r, sz);
    return VF_OK;
}

int vf_engine_read_closure_gate_all(vf_engine* e, int32_t* status, double* nis) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    if (int rc = check_closure_gate(e, 0, "vf_engine_read_closure_gate_all")) return rc;
    const size_t n = (size_t)e->mem.closure_gate_count();
    std::vector<vf_closure_gate_result> r(n);
    HIPCHK(hipMemcpyAsync(r.data(), e->cg_out.get(), n * vf::CLOSURE_RECORD, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < n; i++) {
        if (status) status[i] = r[i].status;
        if (nis) nis[i] = r[i].nis;
    }
    return VF_OK;
}

int vf_engine_closure_gate_status(vf_engine* e, float* h2d_ms, float* kernel_ms, uint64_t* scratch_bytes, uint64_t* result_bytes) {
    VF_ENTER(e, Entry::reads, Entry::leaves_result);
    HIPCHK(e->closure.timings(h2d_ms, kernel_ms));
    if (scratch_bytes) *scratch_bytes = e->cg_scratch.bytes() + e->cg_aux.bytes();
    if (result_bytes) *result_bytes = e->cg_out.bytes();
    return VF_OK;
}
