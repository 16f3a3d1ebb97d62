// engine/engine_marginals.inc -- marginal covariances of the solved keyframes (vf_engine_marginals / vf_engine_read_marginals).
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.
//
// The undamped factorisation at the current states is launched on vf::undamped_whole (vf_launch_view.hpp): the engine's View with
// lambda, failure flags and `fresh` flags pointing at arrays of this section.  The LM state of the engine (states, increments, lambda, counters, done flags, sticky words,
// the cached result block) is not touched.  What is overwritten -- the current buffer's linearisation (the same bits: it is of
// the same states), H, g and the panels -- is what a cold start rebuilds, and the engine is marked cold.
//
// VF_MARGINALS_FAR: far factors alive are taken in as the low-rank downdate of k4_selinv_far.inc, after k_band_selinv.  Their
// lists and the linear far factor are only read (the current buffer's far linearisation is rewritten, with the same bits as
// the rest of it); the scratch is this section's own (fc_scratch), never far_scratch, x_Z, x_gtmp or the column engine's.
// Z takes M x 15 x m doubles per window: at most FARCOV_BUDGET bytes of windows are done at a time, in groups.  Each group costs
// the latency of its substitution chains (two dependent steps per keyframe) whatever its size, so a group should hold every window
// the GPU can run at once.  1 GiB holds one far factor per window on a 1 024-window engine of 1 088 slots (0.8 GB, as much as the
// solve's own Woodbury columns take on that engine, x_Z): that case is one group.  With eight closures per window (m = 48) it
// makes groups of about 180 windows of 1 024 slots instead of asking for 6 GB.
constexpr size_t FARCOV_BUDGET = (size_t)1 << 30;
// VF_MARGINALS_TAIL: the selected inversion stops after the last two keyframes of every window -- what the innovation gate reads
// (engine/engine_gate.inc).  sig_lo says so, and every reader's range check refuses what was not computed.
constexpr int MARGINALS_TAIL_DEPTH = 2;
// The front half of vf_engine_marginals_ex, which vf_engine_gate_closures (engine/engine_closure.inc) shares: the linearisation at
// the current states, the far factors' too where any is alive (e->x_used, recounted by the caller), and the undamped sweep of
// every window whole; `a` is the view it ran on.  zero / failed / ones: [B] each -- a zero lambda, the failure flags (cleared
// here, set by the sweep) and all-ones `fresh` flags, the caller's own.
static int factor_undamped(vf_engine* e, double* zero, int* failed, int* ones, vf::View* out) {
    e->mem.rewritten();
    // undamped, every window assembled and swept whole -- whether or not the termination rule has finished it, whatever form the
    // engine's solves take (they may be partitioned)
    const vf::View a = vf::undamped_whole(e->v, zero, failed, ones);
    HIPCHK(hipMemsetAsync(failed, 0, (size_t)e->v.B * sizeof(int), e->stream));
    // linearisation at the current states (which = 0): the estimate, or theta of a reference-compat engine
    vf::launch_linearize(a, e->btw_kind, 0, e->stream);
    if (e->x_used > 0) vf::launch_linearize_extra(a, 0, e->stream);     // (launch_linearize leaves the far factors to the caller)
    // the forward sweep of the engine's own solves when they assemble H themselves (form 2), else k_band_forward after K3.  The plan
    // is the one the same engine without far factors would have: far factors veto the assembling sweep for the SOLVE (its Woodbury
    // columns read H and g), but they never enter the band and the downdate reads only the panels -- so a window without far
    // factors gets the bits it gets from an engine that has none, on batch engines that assemble as well
    const vf::SolvePlan plan = vf::solve_plan(solve_inputs(e, false));
    if (plan.factor == vf::Sweep::split) vf::launch_assemble(a, e->stream);
    vf::launch_band_factor(a, plan, e->stream);
    *out = a;
    return VF_OK;
}
int vf_engine_marginals(vf_engine* e) { return vf_engine_marginals_ex(e, 0); }
int vf_engine_marginals_ex(vf_engine* e, unsigned flags) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (flags & ~(unsigned)(VF_MARGINALS_FAR | VF_MARGINALS_POSE | VF_MARGINALS_TAIL)) return fail(VF_ERR_INVALID, "vf_engine_marginals_ex: unknown flags 0x%x", flags);
    const bool far = (flags & VF_MARGINALS_FAR) != 0, pose = (flags & VF_MARGINALS_POSE) != 0, tail = (flags & VF_MARGINALS_TAIL) != 0;
    if (tail && (far || pose))
        return fail(VF_ERR_INVALID, "vf_engine_marginals_ex: VF_MARGINALS_TAIL goes with neither VF_MARGINALS_FAR (the downdate corrects whole windows) nor VF_MARGINALS_POSE (records of every keyframe)");
    Entry entry_(e, Entry::reads, Entry::leaves_result);      // (nothing here touches the result block of the last solve)
    if (int rc = not_sharded(e, "vf_engine_marginals")) return rc;
    e->recount_far();
    if (e->x_used > 0 && !far)
        return fail(VF_ERR_INVALID, "vf_engine_marginals: a window holds far factors (vf_engine_get_extra_between / vf_engine_get_linear_far); "
                    "their correction of the covariance needs vf_engine_marginals_ex(e, VF_MARGINALS_FAR)");
    e->mem.covariances_started();      // (behind every refusal: a refused call leaves the engine as it was)
    const int m = 6 * e->x_used;
    const size_t zwin = (size_t)e->v.M * 15 * m, cwin = (size_t)m * m;
    int group = 0;
    if (m > 0) {
        const size_t per = (zwin + cwin) * sizeof(double);
        group = (int)std::max<size_t>(1, std::min<size_t>((size_t)e->v.B, FARCOV_BUDGET / per));
        const size_t want = (size_t)group * per;
        if (want > e->fc_scratch.bytes()) {
            HIPCHK(hipStreamSynchronize(e->stream));
            HIPCHK(e->fc_scratch.ensure(want));
        }
    }
    const size_t G = (size_t)e->v.G, B = (size_t)e->v.B;
    if (!e->sig) {
        // allocated on first use (G x 2.7 KB): engines that never ask for covariances do not grow
        HIPCHK(e->sig.ensure(G * vf::SIG_SLOT * sizeof(double) + B * (sizeof(double) + 2 * sizeof(int)) + 256));
        std::vector<int> ones(B, 1);
        HIPCHK(hipMemsetAsync(e->sig_zero(), 0, B * sizeof(double), e->stream));
        HIPCHK(hipMemcpyAsync(e->sig_ones(), ones.data(), B * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    // allocated on first use as sig is (G x 624 B): only engines that ask for the nav_msgs records hold them
    if (pose) HIPCHK(e->pm_cov.ensure(G * (36 + 36 + 6) * sizeof(double) + 2 * B * sizeof(int) + 256));
    vf::View a{};
    if (int rc = factor_undamped(e, e->sig_zero(), e->sig_fail(), e->sig_ones(), &a)) return rc;
    vf::launch_selinv(a, e->sig_fail(), e->sig, tail ? MARGINALS_TAIL_DEPTH : 0, e->stream);
    for (int w0 = 0; w0 < e->v.B && m > 0; w0 += group) {
        vf::FarCov fc{};
        fc.Z = e->fc_scratch;
        fc.C = e->fc_scratch + (size_t)group * zwin;
        fc.failed = e->sig_fail();
        fc.w0 = w0;
        fc.m = m;
        fc.slots = e->x_used;
        fc.zwin = zwin;
        fc.cwin = cwin;
        vf::launch_farcov(a, fc, std::min(group, e->v.B - w0), e->sig, e->stream);
    }
    // the nav_msgs records of every keyframe, of the states this call linearised at (they may move before anyone reads)
    if (pose) vf::launch_pose_marginals(a, e->sig_fail(), e->sig, e->pm_cov, e->pm_info(), e->pm_pose(), e->pm_range(), e->stream);
    HIPCHK(hipGetLastError());
    e->sig_lo = e->h_lo;
    e->sig_hi = e->h_hi;
    for (int w = 0; w < e->v.B && tail; w++) e->sig_lo[w] = std::max(e->h_lo[w], e->h_hi[w] - MARGINALS_TAIL_DEPTH);
    if (tail) e->mem.covariances_computed_tail();
    else e->mem.covariances_computed(pose);
    return VF_OK;
}

// What every reader of the results refuses, in this order: a window that is not there; results that are not (need 0: the
// blocks, 1: the pose records too, 2: and scores of them); keyframes outside the range they were computed for; a window whose
// factorisation failed (the one synchronisation of a read).
static int check_marginals(vf_engine* e, int window, int k0, int n, int need, const char* what) {
    if (int rc = check_window(e, window)) return rc;
    if (need == 2 && e->mem.score_rows() == 0)
        return fail(VF_ERR_INVALID, "%s: no scores: call vf_engine_marginal_scores after vf_engine_marginals_ex with VF_MARGINALS_POSE", what);
    if (!e->mem.covariances_valid()) return fail(VF_ERR_INVALID, "%s: no marginal covariances: call vf_engine_marginals_ex first", what);
    if (need && !e->mem.pose_records_valid()) return fail(VF_ERR_INVALID, "%s: the last vf_engine_marginals_ex did not carry VF_MARGINALS_POSE", what);
    if (n < 0 || k0 < e->sig_lo[window] || k0 + n > e->sig_hi[window])
        return fail(VF_ERR_BAD_KEY, "%s: keyframes [%d,%d) outside the range [%d,%d) the covariances were computed for", what, k0, k0 + n,
                    e->sig_lo[window], e->sig_hi[window]);
    int failed = 0;
    HIPCHK(hipMemcpyAsync(&failed, e->sig_fail() + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (failed) return fail(VF_ERR_NOT_SPD, "window %d: the undamped normal equations are not positive definite", window);
    return VF_OK;
}

int vf_engine_read_marginals(vf_engine* e, int window, int k0, int n, double* cov225, double* cross225) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_marginals(e, window, k0, n, 0, "vf_engine_read_marginals")) return rc;
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

int vf_engine_read_pose_marginals(vf_engine* e, int window, int k0, int n, double* cov36, double* info36, double* pose6) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_marginals(e, window, k0, n, 1, "vf_engine_read_pose_marginals")) return rc;
    if (n == 0) return VF_OK;
    const size_t g = (size_t)window * e->v.M + k0;
    if (cov36) HIPCHK(hipMemcpy(cov36, e->pm_cov + g * 36, (size_t)n * 36 * sizeof(double), hipMemcpyDeviceToHost));
    if (info36) HIPCHK(hipMemcpy(info36, e->pm_info() + g * 36, (size_t)n * 36 * sizeof(double), hipMemcpyDeviceToHost));
    if (pose6) HIPCHK(hipMemcpy(pose6, e->pm_pose() + g * 6, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    return VF_OK;
}

// K6 on those records, every window's range a series of its own (vf_degeneracy.hip, k_degeneracy_scores_windows).  Enqueues.
int vf_engine_marginal_scores(vf_engine* e, int source, int metric, unsigned subset_mask) {
    VF_ENTER(e, Entry::reads, Entry::leaves_result);
    if (source != VF_SCORE_COVARIANCE && source != VF_SCORE_INFORMATION)
        return fail(VF_ERR_INVALID, "vf_engine_marginal_scores: source must be VF_SCORE_COVARIANCE or VF_SCORE_INFORMATION");
    if (metric < 0 || metric >= vf::K6_METRICS) return fail(VF_ERR_INVALID, "vf_engine_marginal_scores: unknown metric %d", metric);
    if (subset_mask == 0 || (subset_mask >> vf::K6_SUBSETS) != 0)
        return fail(VF_ERR_INVALID, "vf_engine_marginal_scores: subset_mask 0x%x: bits 0 .. 8, at least one", subset_mask);
    if (!e->mem.pose_records_valid())
        return fail(VF_ERR_INVALID, "vf_engine_marginal_scores: no pose marginals (vf_engine_marginals_ex with VF_MARGINALS_POSE; compact and grow void them)");
    const int rows = __builtin_popcount(subset_mask);
    const size_t want = (size_t)rows * e->v.G * sizeof(double);
    e->mem.scores_computed(0);
    if (want > e->sc.bytes()) {
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(e->sc.ensure(want));
    }
    vf::launch_degeneracy_scores_windows(metric, subset_mask, source == VF_SCORE_COVARIANCE ? e->pm_cov.get() : e->pm_info(), e->pm_pose(), e->pm_range(),
                                         e->v.B, e->v.M, e->sc, e->stream);
    HIPCHK(hipGetLastError());
    e->mem.scores_computed(rows);
    return VF_OK;
}

int vf_engine_read_marginal_scores(vf_engine* e, int window, int k0, int n, double* out) {
    Entry entry_(e, Entry::reads);
    if (int rc = check_marginals(e, window, k0, n, 2, "vf_engine_read_marginal_scores")) return rc;
    if (n == 0 || !out) return VF_OK;
    // row r of the scores holds G values, a keyframe's at its slot: one strided copy of `rows` stretches of n
    HIPCHK(hipMemcpy2D(out, (size_t)n * sizeof(double), e->sc + (size_t)window * e->v.M + k0, (size_t)e->v.G * sizeof(double),
                       (size_t)n * sizeof(double), (size_t)e->mem.score_rows(), hipMemcpyDeviceToHost));
    return VF_OK;
}
