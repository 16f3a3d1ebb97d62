// engine/engine_staging.inc -- host -> device staging of states and factors, asynchronous staging, ingest.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// Warm start across the GraphManager's call sequence (vf_solve: preintegrate / predict / set_between for the NEW keyframes,
// marginalize + drop_oldest for the ones that leave, set_range): a call that only touches keyframe slots at or beyond the
// window's current end leaves every existing record, H row and g entry those of the current states, exactly as
// vf_engine_slide does -- the next vf_engine_iterate then linearises only what was appended (k_linearize_tail).  Such calls
// enter with Entry::appends(window, first slot); the rule itself is SolveMemory::written_from.
static int not_sharded(vf_engine* e, const char* what) {
    if (e->v.sh_G > 1)
        return fail(VF_ERR_INVALID, "%s works on whole windows; this engine holds shard %d of %d (use the staged calls, "
                    "include/vilfusion.h \"time-sharded windows\")", what, e->v.sh_r, e->v.sh_G);
    return VF_OK;
}
// What vf_engine_propagate_tail and vf_engine_gate_tail (`who`) ask alike: whole windows, offsets from 0 that do not decrease, no empty
// window and, where the call reads the marginal covariances (cov_needs: how `who` says so), that they are valid and cover the last keyframe
static int check_tail_steps(vf_engine* e, const char* who, const int32_t* step_off, const double* steps, const char* cov_needs) {
    if (int rc = not_sharded(e, who)) return rc;
    const int B = e->v.B;
    if (step_off[0] != 0 || (step_off[B] > 0 && !steps)) return fail(VF_ERR_INVALID, "bad step offsets");
    if (cov_needs && !e->mem.covariances_valid()) return fail(VF_ERR_INVALID, "%s: %s", who, cov_needs);
    for (int w = 0; w < B; w++) {
        if (step_off[w + 1] < step_off[w]) return fail(VF_ERR_INVALID, "bad step offsets (window %d)", w);
        const int hi = e->h_hi[w], lo = e->h_lo[w];
        if (hi <= lo) return fail(VF_ERR_BAD_KEY, "window %d is empty", w);
        if (cov_needs && (hi - 1 < e->sig_lo[w] || hi > e->sig_hi[w]))
            return fail(VF_ERR_INVALID, "%s: window %d: the covariances were computed for the keyframes [%d,%d), the last keyframe is %d",
                        who, w, e->sig_lo[w], e->sig_hi[w], hi - 1);
    }
    return VF_OK;
}
static int check_window(vf_engine* e, int window) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (window < 0 || window >= e->v.B) return fail(VF_ERR_INVALID, "window %d out of range", window);
    return VF_OK;
}
static int check_range(vf_engine* e, int window, int k0, int n) {
    int rc = check_window(e, window);
    if (rc) return rc;
    if (k0 < 0 || n < 0 || k0 + n > e->v.M) return fail(VF_ERR_BAD_KEY, "keyframes [%d,%d) outside capacity %d", k0, k0 + n, e->v.M);
    return VF_OK;
}

int vf_engine_set_range(vf_engine* e, int window, int lo, int hi) {
    Entry entry_(e, Entry::reads);
    // (inherited order: a bad argument is a rewrite, like any call the bookkeeping cannot follow)
    int rc = check_window(e, window);
    if (rc) { if (e) e->mem.rewritten(); return rc; }
    if (lo < 0 || hi < lo || hi > e->v.M) { e->mem.rewritten(); return fail(VF_ERR_BAD_KEY, "bad range [%d,%d)", lo, hi); }
    e->mem.range_set(lo, hi, e->h_lo[window], e->h_hi[window]);
    if (e->async_base()) {
        vf::launch_set_range(e->v, window, lo, hi, e->stream);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemcpyAsync(e->v.lo + window, &lo, sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->v.hi + window, &hi, sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    e->h_lo[window] = lo;
    e->h_hi[window] = hi;
    return VF_OK;
}
int vf_engine_set_async(vf_engine* e, int on) {
    VF_ENTER(e, Entry::reads);
    if (on) { int rc; if ((rc = e->ensure_async()) || (rc = e->ensure_side())) return rc; }
    e->async_on = on != 0;
    return VF_OK;
}
int vf_engine_read_result(vf_engine* e, int window, int slot, int estimate, double* state16, double* cost, int* accepted, int* rejected,
                          int* solve_failures, int* device_flags) {
    Entry entry_(e, Entry::reads, Entry::leaves_result);
    const bool cached = e && e->mem.result_cached_for(window, slot, estimate != 0);
    if (e) e->mem.entry_ran(false);      // (this read, like any other call, ends the cache)
    int rc = check_range(e, window, slot, 1);
    if (rc) return rc;
    if ((rc = e->ensure_async())) return rc;
    if (!cached) {
        vf::launch_read_result(e->v, window, slot, estimate ? 1 : 0, e->sticky_dev, e->res_host, e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    vf::SolveResult& r = *e->res_host;
    e->mem.sticky_handed_on(&r.sticky[0], &r.sticky[1]);
    if (state16) memcpy(state16, r.state, sizeof(r.state));
    if (cost) *cost = r.cost;
    if (accepted) *accepted = r.n_acc;
    if (rejected) *rejected = r.n_rej;
    if (solve_failures) *solve_failures = r.n_fail;
    if (device_flags) *device_flags = (r.sticky[0] ? 1 : 0) | (r.sticky[1] & 4 ? 4 : (r.sticky[1] ? 2 : 0));
    return VF_OK;
}

int vf_engine_set_states(vf_engine* e, int window, int k0, int n, const double* s) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (!s) return fail(VF_ERR_INVALID, "null states");
    if (n == 0) return VF_OK;
    const size_t bytes = (size_t)n * 16 * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, s, bytes, hipMemcpyHostToDevice, e->stream));
    const long g0 = (long)window * e->v.M + k0;
    // both buffers get the value so that "current" is well defined whatever sel is
    vf::launch_scatter_states(e->stage, e->v.x, e->v.G, 0, g0, n, e->stream);
    vf::launch_scatter_states(e->stage, e->v.x, e->v.G, 1, g0, n, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_get_states(vf_engine* e, int window, int k0, int n, double* s) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (!s) return fail(VF_ERR_INVALID, "null states");
    if (n == 0) return VF_OK;
    const size_t bytes = (size_t)n * 16 * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    const long g0 = (long)window * e->v.M + k0;
    vf::launch_gather_states(e->v.x, e->stage, e->v.G, e->v.sel, e->v.M, 0, g0, n, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s, e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_set_imu(vf_engine* e, int window, int k0, int n, const double* rec) {
    Entry entry_(e, Entry::appends(window, k0));
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (!rec) return fail(VF_ERR_INVALID, "null records");
    if (n == 0) return VF_OK;
    const size_t bytes = (size_t)n * vf::IMU_IN * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    HIPCHK(hipMemcpyAsync(e->stage, rec, bytes, hipMemcpyHostToDevice, e->stream));
    vf::launch_scatter(e->stage, e->v.imu_in, (long)window * e->v.M + k0, n, vf::IMU_IN, e->stream);
    vf::launch_fixed_jwords(e->v, (long)window * e->v.M + k0, n, e->stream);    // (the records' own words of the J stream: K1 does not write them)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_set_between(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec) {
    int first = n > 0 ? 1 << 30 : 0;
    for (int i = 0; i < n && b; i++) first = b[i] < first ? b[i] : first;
    Entry entry_(e, Entry::appends(window, first), Entry::overlaps);
    int rc = check_window(e, window);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!a || !b || !rec))) return fail(VF_ERR_INVALID, "null argument");
    const int M = e->v.M, W = e->opts.bandwidth;
    for (int i = 0; i < n; i++) {
        if (a[i] < 0 || b[i] >= M || a[i] >= b[i]) return fail(VF_ERR_BAD_KEY, "between factor %d: need 0 <= a < b < capacity (a=%d b=%d)", i, a[i], b[i]);
        if (b[i] - a[i] > W) return fail(VF_ERR_CAPACITY, "between factor %d spans %d keyframes > bandwidth %d", i, b[i] - a[i], W);
    }
    if (e->async_base() && n <= 4) {
        // (a record travels as a kernel argument: no staging copy, no synchronisation)
        for (int i = 0; i < n; i++) {
            vf::BtwArg arg;
            memcpy(arg.r, rec + (size_t)i * vf::BTW_IN, sizeof(arg.r));
            vf::launch_put_between(e->v, (long)window * M + b[i], a[i], arg, e->stream);
        }
        if (e->v.btw_loss && n > 0) {              // (a new record is a Gaussian factor until it is given a loss)
            vf::BtwLossArg la{};
            la.n = n;
            for (int i = 0; i < n; i++) la.g[i] = (long)window * M + b[i];
            vf::launch_put_between_loss(e->v, la, e->stream);
        }
        if (e->btw_kind && n > 0) {                // (... and a between factor, whatever the slot held)
            vf::BtwKindArg ka{};
            ka.n = n;
            for (int i = 0; i < n; i++) ka.g[i] = (long)window * M + b[i];
            vf::launch_put_between_kind(e->btw_kind, ka, e->stream);
        }
        HIPCHK(hipGetLastError());
        return VF_OK;
    }
    if (e->side_open) { if (int rj = e->join_side()) return rj; }
    // records go to the slot of b: runs of consecutive b are staged in one scatter
    int i = 0;
    while (i < n) {
        int j = i + 1;
        while (j < n && b[j] == b[j - 1] + 1) j++;
        const int cnt = j - i;
        const size_t bytes = (size_t)cnt * vf::BTW_IN * sizeof(double);
        if ((rc = e->ensure_stage(bytes))) return rc;
        HIPCHK(hipMemcpyAsync(e->stage, rec + (size_t)i * vf::BTW_IN, bytes, hipMemcpyHostToDevice, e->stream));
        const long g0 = (long)window * M + b[i];
        vf::launch_scatter(e->stage, e->v.btw_in, g0, cnt, vf::BTW_IN, e->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(e->v.btw_a + g0, a + i, cnt * sizeof(int), hipMemcpyHostToDevice, e->stream));
        if ((rc = e->reset_loss(g0, cnt))) return rc;
        HIPCHK(hipStreamSynchronize(e->stream));
        i = j;
    }
    return VF_OK;
}

// A window's far list, replaced as a whole: the entries and, with them, their robust losses (loss / k null: every entry Gaussian,
// vf_engine_set_extra_between; the arguments of vf_engine_set_extra_between_robust have been checked by it).  Every place that
// rebuilds a list -- transport_far, vf_engine_compact, vf_engine_grow -- comes through here with the losses of the entries it keeps.
static int set_far_list(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec, const int32_t* loss, const double* k) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_window(e, window);
    if (rc) return rc;
    if (int rs = not_sharded(e, "vf_engine_set_extra_between")) return rs;
    if (n < 0 || n + e->h_ln(window) > e->x_cap)
        return fail(VF_ERR_CAPACITY, "at most %d far between factors per window (got %d, and %d carried on from keyframes that have been marginalised; "
                    "vf_engine_opts.max_far_factors raises the bound to %d)", e->x_cap, n, e->h_ln(window), VF_MAX_FAR_LIMIT);
    if (n > 0 && (!a || !b || !rec)) return fail(VF_ERR_INVALID, "null argument");
    const int M = e->v.M, B = e->v.B, X = e->x_cap;
    for (int i = 0; i < n; i++) {
        if (a[i] < 0 || b[i] >= M || a[i] >= b[i]) return fail(VF_ERR_BAD_KEY, "far between factor %d: need 0 <= a < b < capacity (a=%d b=%d)", i, a[i], b[i]);
        if (!(rec[(size_t)i * vf::BTW_IN + 7] > 0.0)) return fail(VF_ERR_NOT_SPD, "far between factor %d: singular square-root information", i);
    }
    if (e->v.x_max == 0 && n == 0) return VF_OK;
    // the losses as the engine keeps them: one id and one parameter per entry, 0 and 0.0 for an entry without a loss
    std::vector<int> hl(n, VF_LOSS_NONE);
    std::vector<double> hk(n, 0.0);
    bool any_loss = false;
    for (int i = 0; i < n && loss; i++)
        if (loss[i] != VF_LOSS_NONE) { hl[i] = loss[i]; hk[i] = k[i]; any_loss = true; }
    // the list the device holds already (the GraphManager re-sends its far factors at every solve; a slide that converts none
    // re-sends the survivors): nothing to do -- no copies, no synchronisation, the captured launch sequence stays valid
    if (e->v.x_max > 0 && !e->h_xdirty[window] && n == e->h_xn[window] && (n == 0 || (!memcmp(a, e->h_xa[window].data(), n * sizeof(int)) &&
        !memcmp(b, e->h_xb[window].data(), n * sizeof(int)) && !memcmp(rec, e->h_xrec[window].data(), (size_t)n * vf::BTW_IN * sizeof(double)) &&
        !memcmp(hl.data(), e->h_xloss[window].data(), n * sizeof(int)) && !memcmp(hk.data(), e->h_xk[window].data(), n * sizeof(double))))) {
        const int before = e->x_used;
        e->recount_far();                                // (the linear far ends are counted too, and those come and go without this list changing)
        if (e->x_used != before) e->epoch++;
        return VF_OK;
    }
    static const bool timing = getenv("VF_SOLVE_TIMING") != nullptr;
    auto t_a = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (timing) { auto t_b = std::chrono::steady_clock::now(); fprintf(stderr, "[set_extra] %-14s %8.1f us\n", what, std::chrono::duration<double, std::micro>(t_b - t_a).count()); t_a = t_b; } };
    {
        int need = n + e->h_ln(window);                   // slots in use once this call is through
        for (int w = 0; w < B && e->v.x_max; w++) if (w != window) need = std::max(need, e->h_xn[w] + e->h_ln(w));
        if ((rc = e->ensure_far(need))) return rc;
    }
    e->attach_far();
    if (any_loss && (rc = e->ensure_far_loss())) return rc;      // (the first list that carries a loss makes the arrays)
    lap("ensure_far");
    // the column engine holds a copy of the window's H per Woodbury column: sized by the far factors alive (6 columns each), grown
    // by doubling -- one loop closure costs 6 windows (0.14 GB, 2 ms to make at 1 200 slots), not the 48 of VF_MAX_EXTRA (1.3 GB, 13 ms)
    const int far_need = n + e->h_ln(window);
    if (e->far_columns && e->far_columns->v.B < 6 * far_need) { vf_engine_destroy(e->far_columns); e->far_columns = nullptr; }
    if (n > 0 && !e->far_columns && !e->far_columns_off && !e->is_far_columns && B == 1 && e->v.P >= 2 && e->tune.far_batch_columns) {
        vf_engine_opts co = e->opts;
        int slots = 1;
        while (slots < far_need) slots *= 2;
        co.windows = 6 * (slots < e->x_cap ? slots : e->x_cap);
        co.max_far_factors = 0;
        co.capacity = M;
        co.incremental = 0;
        vf_engine_tuning ct = e->tune;
        ct.use_hip_graph = 0;
        vf_engine* c = nullptr;
        if (create_engine(&co, &ct, true, e->stream, &c, B) == VF_OK) {
            lap("create columns");
            c->is_far_columns = true;
            if (c->v.P == e->v.P && c->v.P_fit == e->v.P_fit) e->far_columns = c;
            else vf_engine_destroy(c);
        }
        // (it could not be had -- no memory for it, or not in this engine's form: sequential columns from now on, and no second
        // attempt at every call: making and dropping a 4 GB engine per vf_solve is what a refusal cost before this flag)
        if (!e->far_columns) { e->far_columns_off = true; (void)hipGetLastError(); }
    }
    e->h_xa[window].assign(a, a + n);
    e->h_xb[window].assign(b, b + n);
    e->h_xrec[window].assign(rec, rec + (size_t)n * vf::BTW_IN);
    e->h_xloss[window] = hl;
    e->h_xk[window] = hk;
    std::vector<int> ha(X, -1), hb(X, -1);
    std::vector<double> hr((size_t)X * vf::BTW_IN, 0.0);
    for (int i = 0; i < n; i++) { ha[i] = a[i]; hb[i] = b[i]; }
    if (n) memcpy(hr.data(), rec, (size_t)n * vf::BTW_IN * sizeof(double));
    HIPCHK(hipMemcpyAsync(e->v.x_a + (size_t)window * X, ha.data(), X * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->v.x_b + (size_t)window * X, hb.data(), X * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->v.x_in + (size_t)window * X * vf::BTW_IN, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (e->v.x_loss) {              // (a list without losses on an engine that holds the arrays: NONE everywhere, which is what clears them)
        hl.resize(X, VF_LOSS_NONE);
        hk.resize(X, 0.0);
        HIPCHK(hipMemcpyAsync(e->x_loss_id(window), hl.data(), X * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->x_loss_k(window), hk.data(), X * sizeof(double), hipMemcpyHostToDevice, e->stream));
    }
    // both linearisation buffers of the window start from zeros (an empty slot must read as "no factor")
    for (int bf = 0; bf < 2; bf++)
        HIPCHK(hipMemsetAsync(e->v.x_out + ((size_t)bf * B + window) * X * vf::BTW_OUT, 0, (size_t)X * vf::BTW_OUT * sizeof(double), e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    lap("lists");
    e->h_xn[window] = n;
    e->h_xdirty[window] = 0;
    e->recount_far();
    e->epoch++;        // (the number of band solves per trial is baked into a captured launch sequence)
    return VF_OK;
}

int vf_engine_set_extra_between(vf_engine* e, int window, int n, const int32_t* a, const int32_t* b, const double* rec) {
    return set_far_list(e, window, n, a, b, rec, nullptr, nullptr);
}

int vf_engine_clear_between(vf_engine* e, int window, int k0, int n) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0) return VF_OK;
    HIPCHK(hipMemsetAsync(e->v.btw_a + (long)window * e->v.M + k0, 0xff, n * sizeof(int), e->stream));
    if ((rc = e->reset_loss((long)window * e->v.M + k0, n))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_set_prior(vf_engine* e, int window, int k, const double* rec) {
    Entry entry_(e, Entry::rewrites);
    int rc = check_range(e, window, k, 1);
    if (rc) return rc;
    if (!rec) return fail(VF_ERR_INVALID, "null record");
    for (int i = 0; i < 15; i++)
        if (!(rec[16 + i] > 0.0)) return fail(VF_ERR_NOT_SPD, "prior sigma %d must be > 0", i);
    HIPCHK(hipMemcpyAsync(e->v.prior_in + (size_t)window * vf::PRIOR_IN, rec, vf::PRIOR_IN * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->v.prior_k + window, &k, sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->v.mp_on + window, 0, sizeof(int), e->stream));   // a fresh anchor replaces any marginal prior
    if (e->v.x_max > 0 && e->h_ln(window) > 0) {                               // ... and the linear far factor that is expressed around it
        HIPCHK(hipMemsetAsync(e->v.xl_n + window, 0, sizeof(int), e->stream));
        e->far_ended += e->h_ln(window);
        e->h_lb[window].clear();
        e->recount_far();
        e->epoch++;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_preintegrate(vf_engine* e, int window, int k0, int n, const int32_t* off, const double* steps,
                           const double* bhat, const vf_imu_params* p) {
    Entry entry_(e, Entry::appends(window, k0), Entry::overlaps);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (!off || !bhat || !p) return fail(VF_ERR_INVALID, "null argument");
    if (n == 0) return VF_OK;
    if (k0 < 1) return fail(VF_ERR_BAD_KEY, "imu factor slot 0 does not exist (factor k links k-1 -> k)");
    const int total = off[n];
    if (off[0] < 0 || total < off[0] || (total > 0 && !steps)) return fail(VF_ERR_INVALID, "bad step offsets");
    for (int i = 0; i < n; i++)
        if (off[i + 1] <= off[i]) return fail(VF_ERR_INDETERMINATE, "imu factor for keyframe %d has no IMU steps", k0 + i);
    if (e->async_base() && k0 >= e->h_hi[window]) {
        // asynchronous staging: the arguments travel through the pinned block of vf_engine_ingest_tail in ONE copy, the status
        // goes into the sticky word (vf_engine_read_result); nothing here waits for the device
        vf::Packed blk;       // [steps 7 x total][bias 6 x n][offsets n + 1]
        const size_t steps_at = blk.add((size_t)(total > 0 ? total : 1) * 7 * sizeof(double)), bias_at = blk.add((size_t)n * 6 * sizeof(double));
        const size_t off_at = blk.add((size_t)(n + 1) * sizeof(int));
        if ((rc = e->ensure_ingest())) return rc;
        char* h = nullptr;
        HIPCHK(e->ingest.open(blk.bytes, &h));
        if (total > 0) memcpy(h + steps_at, steps, (size_t)total * 7 * sizeof(double));
        memcpy(h + bias_at, bhat, (size_t)n * 6 * sizeof(double));
        memcpy(h + off_at, off, (size_t)(n + 1) * sizeof(int));
        HIPCHK(e->ingest.send(blk.bytes, e->stream, false));
        const char* d = e->ingest.device();
        vf::launch_preintegrate(e->v, (long)window * e->v.M + k0, n, (const int*)(d + off_at), (const double*)(d + steps_at), (const double*)(d + bias_at),
                                imu_cov(p), e->sticky_dev, e->stream);
        HIPCHK(hipGetLastError());
        return VF_OK;
    }
    if (e->side_open) { if (int rj = e->join_side()) return rj; }
    // one scratch block: [steps 7 x total][bias 6 x n][offsets n + 1][status]
    const size_t steps_b = (size_t)(total > 0 ? total : 1) * 7 * sizeof(double), bias_b = (size_t)n * 6 * sizeof(double);
    const size_t off_b = ((size_t)(n + 1) * sizeof(int) + 7) & ~(size_t)7;
    if ((rc = e->ensure_pre(steps_b + bias_b + off_b + 8))) return rc;
    double* d_steps = (double*)e->pre_buf.get();
    double* d_bhat = (double*)(e->pre_buf + steps_b);
    int* d_off = (int*)(e->pre_buf + steps_b + bias_b);
    int* d_status = (int*)(e->pre_buf + steps_b + bias_b + off_b);
    HIPCHK(hipMemcpyAsync(d_off, off, (n + 1) * sizeof(int), hipMemcpyHostToDevice, e->stream));
    if (total > 0) HIPCHK(hipMemcpyAsync(d_steps, steps, (size_t)total * 7 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_bhat, bhat, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(d_status, 0, sizeof(int), e->stream));
    vf::launch_preintegrate(e->v, (long)window * e->v.M + k0, n, d_off, d_steps, d_bhat, imu_cov(p), d_status, e->stream);
    HIPCHK(hipGetLastError());
    int status = 0;
    HIPCHK(hipMemcpyAsync(&status, d_status, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (status) return fail(VF_ERR_NOT_SPD, "preintegrated covariance not positive definite");
    return VF_OK;
}

int vf_engine_ingest_tail(vf_engine* e, const int32_t* step_off, const double* steps, const vf_imu_params* p,
                          const int32_t* btw_a, const double* btw_rec) {
    Entry entry_(e, Entry::reads);
    if (!e || !step_off || !p || !btw_a || !btw_rec) return fail(VF_ERR_INVALID, "null argument");
    const int B = e->v.B, M = e->v.M, W = e->opts.bandwidth;
    const int total = step_off[B];
    if (step_off[0] != 0 || (total > 0 && !steps)) return fail(VF_ERR_INVALID, "bad step offsets");
    for (int w = 0; w < B; w++) {
        if (step_off[w + 1] <= step_off[w]) return fail(VF_ERR_INDETERMINATE, "window %d: the new IMU factor has no IMU steps", w);
        const int hi = e->h_hi[w], lo = e->h_lo[w];
        if (hi >= M) return fail(VF_ERR_CAPACITY, "window %d has no free keyframe slot", w);
        if (hi <= lo) return fail(VF_ERR_BAD_KEY, "window %d is empty", w);
        if (btw_a[w] >= 0 && (btw_a[w] >= hi || btw_a[w] < lo)) return fail(VF_ERR_BAD_KEY, "window %d: between factor from keyframe %d outside the window [%d, %d)", w, btw_a[w], lo, hi);
        if (btw_a[w] >= 0 && hi - btw_a[w] > W) return fail(VF_ERR_CAPACITY, "window %d: between factor spans %d keyframes > bandwidth %d", w, hi - btw_a[w], W);
    }
    // one packed block: [offsets B + 1][between sources B][between records 28 B][steps 7 x total]
    vf::Packed blk;
    const size_t rec_b = (size_t)B * vf::BTW_IN * sizeof(double), st_b = (size_t)total * 7 * sizeof(double);
    const size_t off_at = blk.add((size_t)(B + 1) * sizeof(int)), a_at = blk.add((size_t)B * sizeof(int)), rec_at = blk.add(rec_b), st_at = blk.add(st_b);
    if (int rc = e->ensure_ingest()) return rc;
    char* h = nullptr;
    HIPCHK(e->ingest.open(blk.bytes, &h));
    memcpy(h + off_at, step_off, (size_t)(B + 1) * sizeof(int));
    memcpy(h + a_at, btw_a, (size_t)B * sizeof(int));
    memcpy(h + rec_at, btw_rec, rec_b);
    memcpy(h + st_at, steps, st_b);
    HIPCHK(e->ingest.send(blk.bytes, e->stream, true));
    const char* d = e->ingest.device();
    vf::launch_ingest_tail(e->v, (const int*)(d + off_at), (const double*)(d + st_at), (const int*)(d + a_at),
                           (const double*)(d + rec_at), imu_cov(p), e->in_status, e->stream);
    if (e->v.btw_loss) vf::launch_reset_tail_loss(e->v, e->btw_kind, e->stream);     // (the slot a record has just been written to)
    HIPCHK(hipGetLastError());
    HIPCHK(e->ingest.launched(e->stream));
    // Nothing inside any window changed (the records sit in slot hi, beyond every window's end): a warm engine stays warm,
    // the vf_engine_slide that follows appends the keyframe and the next solve linearises it (k_linearize_tail).
    return VF_OK;
}

int vf_engine_ingest_status(vf_engine* e, float* h2d_ms, float* k0_ms) {
    VF_ENTER(e, Entry::reads);
    HIPCHK(e->ingest.timings(h2d_ms, k0_ms));
    if (!e->ingest.outstanding()) return VF_OK;
    int status = 0;
    HIPCHK(hipMemcpy(&status, e->in_status, sizeof(int), hipMemcpyDeviceToHost));
    if (status) {
        HIPCHK(hipMemset(e->in_status, 0, sizeof(int)));
        if (status & 2) return fail(VF_ERR_CAPACITY, "vf_engine_ingest_tail: a window had no free keyframe slot");
        return fail(VF_ERR_NOT_SPD, "vf_engine_ingest_tail: a preintegrated covariance was not positive definite");
    }
    return VF_OK;
}

int vf_engine_get_imu(vf_engine* e, int window, int k0, int n, double* rec) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0 || !rec) return VF_OK;
    const size_t bytes = (size_t)n * vf::IMU_IN * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    vf::launch_gather(e->v.imu_in, e->stage, (long)window * e->v.M + k0, n, vf::IMU_IN, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rec, e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}
