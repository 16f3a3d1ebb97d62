// engine/engine_read.inc -- read-back and measurement.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// ------------------------------------------------------------------ read-back
static int read_sel(vf_engine* e, int window, int* sel) {
    HIPCHK(hipMemcpyAsync(sel, e->v.sel + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_read_imu_lin(vf_engine* e, int window, int which, int k0, int n, double* r15, double* J450) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0) return VF_OK;
    int sel = 0;
    if ((rc = read_sel(e, window, &sel))) return rc;
    const int b = sel ^ (which ? 1 : 0);
    const size_t bytes = (size_t)n * vf::IMU_OUT * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    vf::launch_gather_imu_lin(e->v, b, (long)window * e->v.M + k0, n, e->stage, e->stream);
    HIPCHK(hipGetLastError());
    std::vector<double> h((size_t)n * vf::IMU_OUT);
    HIPCHK(hipMemcpyAsync(h.data(), e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; i++) {
        if (r15) memcpy(r15 + (size_t)i * 15, h.data() + (size_t)i * vf::IMU_OUT, 15 * sizeof(double));
        if (J450) memcpy(J450 + (size_t)i * 450, h.data() + (size_t)i * vf::IMU_OUT + 15, 450 * sizeof(double));
    }
    return VF_OK;
}

int vf_engine_read_between_lin(vf_engine* e, int window, int which, int k0, int n, double* r6, double* Ja, double* Jb) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0) return VF_OK;
    int sel = 0;
    if ((rc = read_sel(e, window, &sel))) return rc;
    const int b = sel ^ (which ? 1 : 0);
    const size_t bytes = (size_t)n * vf::BTW_OUT * sizeof(double);
    if ((rc = e->ensure_stage(bytes))) return rc;
    const double* src = e->v.btw_out + (size_t)b * (size_t)(e->v.G / 64) * vf::BTW_OUT * 64;
    vf::launch_gather(src, e->stage, (long)window * e->v.M + k0, n, vf::BTW_OUT, e->stream);
    HIPCHK(hipGetLastError());
    std::vector<double> h((size_t)n * vf::BTW_OUT);
    HIPCHK(hipMemcpyAsync(h.data(), e->stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; i++) {
        const double* p = h.data() + (size_t)i * vf::BTW_OUT;
        if (r6) memcpy(r6 + (size_t)i * 6, p, 6 * sizeof(double));
        if (Ja) memcpy(Ja + (size_t)i * 36, p + 6, 36 * sizeof(double));
        if (Jb) memcpy(Jb + (size_t)i * 36, p + 42, 36 * sizeof(double));
    }
    return VF_OK;
}

int vf_engine_read_normal(vf_engine* e, int window, int k0, int n, double* Hband, double* g15) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0) return VF_OK;
    const size_t g0 = (size_t)window * e->v.M + k0;
    if (solve_plan(e).k3 != vf::K3::all) {
        // H and g are not kept by the solves of this engine: assemble them now, for this window only, whether or not the
        // termination rule has finished it (a converged window's H is what Engine.pose_information is asked for)
        vf::launch_assemble_window(e->v, window, e->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (Hband) {
        // device rows are packed for the solver (vf_kernels.hpp "Block row of H") -> the documented [n][4][15][15]
        std::vector<double> raw((size_t)n * vf::HROW);
        HIPCHK(hipMemcpy(raw.data(), e->v.H + g0 * vf::HROW, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::fill(Hband, Hband + (size_t)n * 900, 0.0);
        for (int k = 0; k < n; k++) {
            const double* r = raw.data() + (size_t)k * vf::HROW;
            double* o = Hband + (size_t)k * 900;
            for (int a = 0; a < 15; a++)
                for (int c = 0; c < 15; c++) {
                    o[a * 15 + c] = r[vf::H_D0 + (a >= c ? vf::h_tri(a, c) : vf::h_tri(c, a))];
                    o[225 + a * 15 + c] = r[vf::H_D1 + a * 15 + c];
                }
            for (int a = 0; a < 6; a++) {
                for (int c = 0; c < 6; c++) {
                    o[450 + a * 15 + c] = r[vf::H_D2 + a * 6 + c];
                    o[675 + a * 15 + c] = r[vf::H_D3 + a * 6 + c];
                }
                for (int c = 0; c < 9; c++) o[450 + a * 15 + 6 + c] = r[vf::H_DX + a * 9 + c];
            }
        }
    }
    if (g15) HIPCHK(hipMemcpy(g15, e->v.gvec + g0 * 15, (size_t)n * 15 * sizeof(double), hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_engine_read_delta(vf_engine* e, int window, int k0, int n, double* d) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0 || !d) return VF_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(d, e->v.delta + ((size_t)window * e->v.M + k0) * 15, (size_t)n * 15 * sizeof(double), hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_engine_read_panels(vf_engine* e, int window, int k0, int n, double* panels) {
    Entry entry_(e, Entry::reads);
    int rc = check_range(e, window, k0, n);
    if (rc) return rc;
    if (n == 0 || !panels) return VF_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    // packed device layout (vf_kernels.hpp "Cholesky panel") -> the documented [43][16] (column 15 = 0)
    std::vector<double> raw((size_t)n * vf::PANEL);
    HIPCHK(hipMemcpy(raw.data(), e->v.Lp + ((size_t)window * e->v.M + k0) * vf::PANEL, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++)
        for (int r = 0; r < 43; r++)
            for (int c = 0; c < 16; c++) {
                double x = 0.0;
                if (c < 15) { const int i = vf::panel_idx(r, c); x = i == vf::PANEL_DUMP ? 0.0 : raw[(size_t)k * vf::PANEL + i]; }
                panels[(size_t)k * 688 + r * 16 + c] = x;
            }
    return VF_OK;
}

int vf_engine_read_lm(vf_engine* e, int window, double* cost, double* lambda, int* acc, int* rej, int* fails) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (cost) HIPCHK(hipMemcpy(cost, e->v.cost + window, sizeof(double), hipMemcpyDeviceToHost));
    if (lambda) HIPCHK(hipMemcpy(lambda, e->v.lambda + window, sizeof(double), hipMemcpyDeviceToHost));
    if (acc) HIPCHK(hipMemcpy(acc, e->v.n_acc + window, sizeof(int), hipMemcpyDeviceToHost));
    if (rej) HIPCHK(hipMemcpy(rej, e->v.n_rej + window, sizeof(int), hipMemcpyDeviceToHost));
    if (fails) HIPCHK(hipMemcpy(fails, e->v.n_fail + window, sizeof(int), hipMemcpyDeviceToHost));
    return VF_OK;
}

// ------------------------------------------------------------------ measurement
int vf_engine_read_excursions(vf_engine* e, int window, int* provisional_trials, int* open_now) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    int np = 0, pr = 0;
    if (e->v.x_best) {
        HIPCHK(hipMemcpyAsync(&np, e->v.n_prov + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&pr, e->v.prov + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (provisional_trials) *provisional_trials = np;
    if (open_now) *open_now = pr;
    return VF_OK;
}
int vf_engine_time_stage(vf_engine* e, int stage, int reps, float* avg_ms) {
    Entry entry_(e, Entry::rewrites);
    if (!e || !avg_ms || reps < 1) return fail(VF_ERR_INVALID, "bad argument");
    const vf::View tv = vf::every_window(e->v);      // stage timings are of the full work, whatever the windows' convergence flags say
    // K4's stage is the form the View alone gives: never the hybrid, and the assembling sweep even where the engine's own solves
    // are vetoed from it
    vf::SolveInputs in = solve_inputs(e);
    in.hybrid = false;
    in.vetoed = false;
    const vf::SolvePlan plan = vf::solve_plan(in);
    auto run = [&]() {
        switch (stage) {
            case VF_STAGE_LINEARIZE_IMU: vf::launch_linearize_imu(tv, 0, e->stream); break;
            case VF_STAGE_LINEARIZE_BTW: vf::launch_linearize_between(tv, e->btw_kind, 0, e->stream); break;
            case VF_STAGE_ASSEMBLE: vf::launch_assemble(tv, e->stream); break;
            case VF_STAGE_SOLVE: vf::launch_band_solve(tv, tv, plan, e->stream); break;
            case VF_STAGE_RETRACT: vf::launch_retract(tv, e->stream); break;
            case VF_STAGE_DECIDE: vf::launch_decide(tv, 1, e->stream); break;
            case VF_STAGE_ASSEMBLE_IDLE: vf::launch_assemble(tv, e->stream); break;
            default: break;
        }
    };
    if (stage < VF_STAGE_LINEARIZE_IMU || stage > VF_STAGE_ASSEMBLE_IDLE) return fail(VF_ERR_INVALID, "unknown stage %d", stage);
    // time the full-work form of K3 (inside iterate() it is skipped for windows whose last trial was rejected)
    if (stage == VF_STAGE_ASSEMBLE) HIPCHK(hipMemsetAsync(e->v.fresh, 0x01, e->v.B * sizeof(int), e->stream));
    if (stage == VF_STAGE_ASSEMBLE_IDLE) HIPCHK(hipMemsetAsync(e->v.fresh, 0, e->v.B * sizeof(int), e->stream));
    run();  // warm
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; i++) run();
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *avg_ms = ms / reps;
    if (stage == VF_STAGE_ASSEMBLE_IDLE) HIPCHK(hipMemsetAsync(e->v.fresh, 0x01, e->v.B * sizeof(int), e->stream));   // H is as it was
    return VF_OK;
}

int vf_engine_time_iterate(vf_engine* e, int iterations, float* ms) {
    Entry entry_(e, Entry::rewrites);
    if (!e || !ms) return fail(VF_ERR_INVALID, "bad argument");
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    int rc = vf_engine_iterate(e, iterations);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    HIPCHK(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return VF_OK;
}

int vf_engine_counts(vf_engine* e, int64_t* n_imu, int64_t* n_btw, int64_t* n_kf) {
    VF_ENTER(e, Entry::reads);
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<int> a((size_t)e->v.G);
    HIPCHK(hipMemcpy(a.data(), e->v.btw_a, a.size() * sizeof(int), hipMemcpyDeviceToHost));
    int64_t ni = 0, nb = 0, nk = 0;
    for (int w = 0; w < e->v.B; w++) {
        const int lo = e->h_lo[w], hi = e->h_hi[w];
        if (hi <= lo) continue;
        nk += hi - lo;
        ni += hi - lo - 1;
        for (int k = lo + 1; k < hi; k++) {
            const int aa = a[(size_t)w * e->v.M + k];
            if (aa >= lo && aa < k) nb++;
        }
    }
    if (n_imu) *n_imu = ni;
    if (n_btw) *n_btw = nb;
    if (n_kf) *n_kf = nk;
    return VF_OK;
}
