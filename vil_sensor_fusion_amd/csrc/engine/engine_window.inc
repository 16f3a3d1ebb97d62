// engine/engine_window.inc -- the fixed-lag window: marginalisation (and ahead of time), far factors across a slide, slide, compaction, growth.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
int vf_engine_marginalize(vf_engine* e) {
    VF_ENTER(e, Entry::reads, Entry::overlaps_if(e && e->async_now()));
    // (reads the current linearisation, writes the marginal prior: what a warm start expects to have changed)
    if (int rc = not_sharded(e, "vf_engine_marginalize")) return rc;
    for (int w = 0; w < e->v.B; w++)
        if (e->h_hi[w] - e->h_lo[w] < 4) return fail(VF_ERR_INVALID, "window %d: marginalisation needs >= 4 keyframes", w);
    if (e->async_now() && e->mem.stash_fits(e->h_lo[0])) {
        // computed behind the previous solve (vf_engine_marginalize_ahead, on the side stream): put in place
        if (e->side_open) { if (int rj = e->join_side()) return rj; }
        vf::launch_marg_commit(e->v, e->marg_stash, e->stream);
        HIPCHK(hipGetLastError());
        e->mem.stash_committed();
        e->marg_since_drop = true;
        return VF_OK;
    }
    // (k_marginalize<FAR> strikes the far factors it converts out of the device's list: the host's copy follows in transport_far)
    for (int w = 0; w < e->v.B && e->x_used > 0; w++)
        for (int i = 0; i < e->h_xn[w]; i++)
            if (e->h_xa[w][i] == e->h_lo[w]) e->h_xdirty[w] = 1;
    if (e->async_far()) {
        // far factors alive: on the main stream (the kernel reads and rewrites their lists, which the host re-sends there), behind
        // the linearisation of the ones the prior is about to absorb; what it finds wrong goes into the sticky word
        vf::launch_linearize_extra(vf::every_window(e->v), 0, e->stream);
        vf::launch_marginalize(e->v, e->x_used, e->sticky_dev + 1, e->stream);
        HIPCHK(hipGetLastError());
        e->marg_since_drop = true;
        return VF_OK;
    }
    if (e->async_now()) {
        // beside whatever the main stream is given next (K0, prediction and staging of the keyframe that arrives): a second
        // stream that starts where the main one stands now
        if (!e->side_open) {
            HIPCHK(hipEventRecord(e->ev_fork, e->stream));
            HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
            e->side_open = true;
        }
        vf::launch_marginalize(e->v, e->x_used, e->sticky_dev + 1, e->stream2);
        HIPCHK(hipGetLastError());
        e->marg_since_drop = true;
        return VF_OK;
    }
    HIPCHK(hipMemsetAsync(e->status_dev, 0, sizeof(int), e->stream));
    // far factors the prior is about to absorb: their linearisation at the current states (a compaction, a transport or any
    // other re-sending of the list since the last solve has zeroed the buffers)
    // (a window the termination rule finished in the last solve still has its `done` flag up: linearise it all the same)
    if (e->x_used > 0) vf::launch_linearize_extra(vf::every_window(e->v), 0, e->stream);
    vf::launch_marginalize(e->v, e->x_used, e->status_dev, e->stream);
    HIPCHK(hipGetLastError());
    int status = 0;
    HIPCHK(hipMemcpyAsync(&status, e->status_dev, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (status & 4) return fail(VF_ERR_INDETERMINATE, "marginalisation: the far ends' block of the marginal is not positive definite");
    if (status) return fail(VF_ERR_INDETERMINATE, "marginalisation: pivot block of the oldest keyframe not positive definite");
    e->marg_since_drop = true;
    return VF_OK;
}

// ---- far between factors across a slide: the host's side of what k_marginalize<FAR> has just done on the device.  A far
// factor (a -> b) whose older keyframe a has been MARGINALISED was marginalised with it: it is part of the window's linear far
// factor now (View::xl_*), or -- with its far end within the new prior's reach -- inside the prior; the lists here are host
// mirrors and apply the same rule in the same order (survivors of the linear list, then the nonlinear entries anchored at the
// leaving keyframe, by index).  The information of a loop closure thereby outlives the keyframe it was anchored on (iSAM2
// keeps every factor for good, GraphManager.cpp:83-88).
// A slide that does NOT marginalise (re-anchoring: the keyframe is dropped, its band factors with it) re-anchors a nonlinear
// far factor on the next keyframe instead: with D = T_a^-1 T_a+1 at the current estimate, the measurement Z of T_a^-1 T_b becomes
// Z' = D^-1 Z of T_a+1^-1 T_b -- the same residual Log(Z^-1 T_a^-1 T_b), in the same tangent frame (at b), so the square-root
// information stays as it is; D is known from the IMU factor between the two keyframes to ~2e-5 m / 2e-4 rad, against the
// 1e-2 ... 0.5 m a between factor claims, and is taken as exact (two states are read back per window that has such a factor).
// The linear rows, expressed around the prior that such a slide discards, end there.
namespace {
void quat_to_rot_(const double* q, double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}
void quat_mul_(const double* a, const double* b, double* o) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
}  // namespace
static int transport_far(vf_engine* e, bool marginalised) {
    if (e->x_used == 0) return VF_OK;
    for (int w = 0; w < e->v.B; w++) {
        const int lo = e->h_lo[w], hi = e->h_hi[w];
        bool any = !e->h_lb[w].empty();
        for (int i = 0; i < e->h_xn[w]; i++) any = any || e->h_xa[w][i] == lo;
        if (!any || hi - lo < 2) continue;
        // (1) the linear far factors -- all of them have the leaving keyframe in their support.  k_marginalize has absorbed the
        // ones that end at lo + 3 and re-expressed the others over the next three keyframes, in this order; without a
        // marginalisation (re-anchoring slide) they go the way the band factors of the dropped keyframe go.
        std::vector<int> lb;
        for (int kb : e->h_lb[w]) {
            if (!marginalised) e->far_ended++;
            else if (kb == lo + 3) e->far_absorbed++;
            else lb.push_back(kb);
        }
        const bool had_linear = !e->h_lb[w].empty();
        // (2) the nonlinear ones anchored at lo
        double st[32], R0[9], qD[4], tD[3], RD[9], qDc[4];
        bool have_D = false;
        std::vector<int> a, b, loss;        // (an entry that stays, re-anchored or not, keeps its loss; one that leaves takes it along)
        std::vector<double> rec, lk;
        for (int i = 0; i < e->h_xn[w]; i++) {
            double r[vf::BTW_IN];
            memcpy(r, e->h_xrec[w].data() + (size_t)i * vf::BTW_IN, sizeof(r));
            int ai = e->h_xa[w][i];
            const int kb = e->h_xb[w][i];
            if (ai == lo) {
                // within the marginal prior's reach (ends at lo+1 .. lo+3): k_marginalize has just absorbed it, like a band
                // factor -- its information lives on in the prior
                if (kb - lo <= 3) { if (marginalised) e->far_absorbed++; else e->far_ended++; continue; }
                // marginalised with its far end inside the window: k_marginalize has made it a linear far factor (exact
                // at the current linearisation), behind the survivors of (1)
                if (marginalised && kb < hi) { lb.push_back(kb); e->far_transported++; continue; }
                // no marginalisation (or an end the window has not reached yet): re-anchored on the next keyframe, the step
                // between the two taken as exact
                if (!have_D) {
                    if (int rc = vf_engine_get_states(e, w, lo, 2, st)) return rc;
                    double qc[4] = {st[0], -st[1], -st[2], -st[3]}, dt[3] = {st[20] - st[4], st[21] - st[5], st[22] - st[6]};     // D = T_lo^-1 T_lo+1
                    quat_to_rot_(st, R0);
                    quat_mul_(qc, st + 16, qD);
                    for (int c = 0; c < 3; c++) tD[c] = R0[0 * 3 + c] * dt[0] + R0[1 * 3 + c] * dt[1] + R0[2 * 3 + c] * dt[2];
                    quat_to_rot_(qD, RD);
                    qDc[0] = qD[0]; qDc[1] = -qD[1]; qDc[2] = -qD[2]; qDc[3] = -qD[3];
                    have_D = true;
                }
                double q2[4], d[3] = {r[4] - tD[0], r[5] - tD[1], r[6] - tD[2]};
                quat_mul_(qDc, r, q2);                                          // R' = R_D^T R_Z
                const double nq = std::sqrt(q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2] + q2[3] * q2[3]);
                for (int c = 0; c < 4; c++) r[c] = q2[c] / nq;
                for (int c = 0; c < 3; c++) r[4 + c] = RD[0 * 3 + c] * d[0] + RD[1 * 3 + c] * d[1] + RD[2 * 3 + c] * d[2];   // t' = R_D^T (t_Z - t_D)
                ai = lo + 1;
                e->far_transported++;
            }
            a.push_back(ai);
            b.push_back(kb);
            rec.insert(rec.end(), r, r + vf::BTW_IN);
            loss.push_back(e->h_xloss[w][i]);
            lk.push_back(e->h_xk[w][i]);
        }
        e->h_lb[w] = lb;
        if (had_linear && !marginalised) HIPCHK(hipMemsetAsync(e->v.xl_n + w, 0, sizeof(int), e->stream));
        if (int rc = set_far_list(e, w, (int)a.size(), a.data(), b.data(), rec.data(), loss.data(), lk.data())) return rc;
    }
    return VF_OK;
}
int vf_engine_get_linear_far(vf_engine* e, int window, int* n, int32_t* far_end) {
    int rc = check_window(e, window);
    if (rc) return rc;
    const int cnt = e->v.x_max ? e->h_ln(window) : 0;
    if (n) *n = cnt;
    for (int i = 0; i < cnt && far_end; i++) far_end[i] = e->h_lb[window][i];
    return VF_OK;
}
int vf_engine_get_extra_between(vf_engine* e, int window, int* n, int32_t* a, int32_t* b, double* rec28, long* transported, long* ended, long* absorbed) {
    int rc = check_window(e, window);
    if (rc) return rc;
    const int cnt = e->v.x_max ? e->h_xn[window] : 0;
    if (n) *n = cnt;
    for (int i = 0; i < cnt; i++) {
        if (a) a[i] = e->h_xa[window][i];
        if (b) b[i] = e->h_xb[window][i];
        if (rec28) memcpy(rec28 + (size_t)i * vf::BTW_IN, e->h_xrec[window].data() + (size_t)i * vf::BTW_IN, sizeof(double) * vf::BTW_IN);
    }
    if (transported) *transported = e->far_transported;
    if (ended) *ended = e->far_ended;
    if (absorbed) *absorbed = e->far_absorbed;
    return VF_OK;
}

int vf_engine_marginalize_ahead(vf_engine* e) {
    VF_ENTER(e, Entry::reads);
    // (a warm engine: its records are those of the current states -- what a marginalisation reads -- and stay so while only
    // appends follow; anything else voids the stash: SolveMemory)
    if (!e->async_now() || !e->mem.is_warm() || e->h_hi[0] - e->h_lo[0] < 4) return VF_OK;
    if (int rc = e->ensure_async()) return rc;
    HIPCHK(e->marg_stash.ensure((size_t)e->v.B * vf::MARG_STASH_DOUBLES * sizeof(double)));
    // on the side stream, behind what the main stream holds now: the preintegration vf_reserve_node enqueues next (main stream)
    // then runs beside it when solves come back to back
    if (int rc = e->ensure_side()) return rc;
    HIPCHK(hipEventRecord(e->ev_fork, e->stream));
    HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
    e->side_open = true;
    vf::launch_marginalize_ahead(e->v, e->sticky_dev + 1, e->marg_stash, e->stream2);
    HIPCHK(hipGetLastError());
    e->mem.stashed(e->h_lo[0]);
    return VF_OK;
}
int vf_engine_drop_oldest(vf_engine* e) {
    VF_ENTER(e, Entry::reads, Entry::overlaps_if(e && e->async_now()));
    if (e->async_now()) {
        for (int w = 0; w < e->v.B; w++)
            if (e->h_hi[w] - e->h_lo[w] < 2) return fail(VF_ERR_INVALID, "window %d too short", w);
        vf::launch_bump_lo(e->v, e->side_open ? e->stream2 : e->stream);       // (behind the marginalisation it follows, wherever that runs)
        HIPCHK(hipGetLastError());
        e->marg_since_drop = false;
        for (int w = 0; w < e->v.B; w++) e->h_lo[w]++;
        return VF_OK;
    }
    if (int rc = transport_far(e, e->marg_since_drop)) return rc;
    e->marg_since_drop = false;
    if (e->async_base()) {          // (far factors alive: their bookkeeping above, the window's first keyframe enqueued like the rest)
        if (e->h_hi[0] - e->h_lo[0] < 2) return fail(VF_ERR_INVALID, "window 0 too short");
        vf::launch_bump_lo(e->v, e->stream);
        HIPCHK(hipGetLastError());
        e->h_lo[0]++;
        return VF_OK;
    }
    for (int w = 0; w < e->v.B; w++) {
        if (e->h_hi[w] - e->h_lo[w] < 2) return fail(VF_ERR_INVALID, "window %d too short", w);
        const int lo = e->h_lo[w] + 1;
        HIPCHK(hipMemcpyAsync(e->v.lo + w, &lo, sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int w = 0; w < e->v.B; w++) e->h_lo[w]++;
    return VF_OK;
}

int vf_engine_slide(vf_engine* e, const double* prior_sigma15, int marginalize) {
    Entry entry_(e, Entry::reads);
    if (!e || !prior_sigma15) return fail(VF_ERR_INVALID, "null argument");
    for (int w = 0; w < e->v.B; w++)
        if (e->h_hi[w] >= e->v.M) return fail(VF_ERR_CAPACITY, "window %d has no free keyframe slot", w);
    if (marginalize) {
        int rc = vf_engine_marginalize(e);
        if (rc) return rc;
    }
    if (int rc = transport_far(e, marginalize != 0)) return rc;
    e->marg_since_drop = false;
    e->mem.slid_by_one();
    // the sigmas are a caller temporary: uploaded (and waited for) only when they differ from what the device already holds, so
    // that a run of updates with the same sigmas -- every fixed-lag loop -- enqueues without a host synchronisation
    const bool fresh_sigma = !e->sigma_valid || memcmp(e->sigma_host, prior_sigma15, sizeof(e->sigma_host)) != 0;
    if (fresh_sigma) {
        HIPCHK(hipMemcpyAsync(e->sigma_dev, prior_sigma15, 15 * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        memcpy(e->sigma_host, prior_sigma15, sizeof(e->sigma_host));
        e->sigma_valid = true;
    }
    vf::launch_slide(e->v, e->sigma_dev, marginalize ? 0 : 1, e->stream);
    HIPCHK(hipGetLastError());
    for (int w = 0; w < e->v.B; w++) { e->h_lo[w]++; e->h_hi[w]++; }
    return VF_OK;
}

int vf_engine_read_marginal(vf_engine* e, int window, int* on, double* xbar48, double* L729, double* eta27) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (on) HIPCHK(hipMemcpy(on, e->v.mp_on + window, sizeof(int), hipMemcpyDeviceToHost));
    if (xbar48) HIPCHK(hipMemcpy(xbar48, e->v.mp_x + (size_t)window * 48, 48 * sizeof(double), hipMemcpyDeviceToHost));
    if (L729) HIPCHK(hipMemcpy(L729, e->v.mp_L + (size_t)window * 729, 729 * sizeof(double), hipMemcpyDeviceToHost));
    if (eta27) HIPCHK(hipMemcpy(eta27, e->v.mp_eta + (size_t)window * 27, 27 * sizeof(double), hipMemcpyDeviceToHost));
    return VF_OK;
}

// Move the live keyframes [shift, M) of every window to [0, M - shift): frees `shift` slots at the
// end.  shift must be a multiple of 64 (whole AoSoA tiles) and <= every window's lo.
int vf_engine_compact(vf_engine* e, int shift) {
    VF_ENTER(e, Entry::rewrites);
    vf::View& v = e->v;
    if (shift <= 0 || shift % 64 != 0 || shift >= v.M) return fail(VF_ERR_INVALID, "shift must be a positive multiple of 64 below the capacity");
    e->mem.compacted();
    for (int w = 0; w < v.B; w++)
        if (e->h_lo[w] < shift) return fail(VF_ERR_BAD_KEY, "window %d: lo %d < shift %d (live keyframes would be lost)", w, e->h_lo[w], shift);
    const size_t keepk = (size_t)(v.M - shift);              // slots kept per window
    // staging buffer: the largest per-window segment moved at once (imu_out tiles)
    constexpr int JNF = vf::JT_STRIDE * (64 / vf::JT) / 64;      // the J stream of 64 slots, counted in "fields" of 64 doubles (292)
    static_assert(JNF * 64 == vf::JT_STRIDE * (64 / vf::JT), "J stream tiles per 64 slots");
    const size_t seg_max = (keepk / 64) * (size_t)(JNF > vf::IMU_IN ? JNF : vf::IMU_IN) * 64;
    int rc = e->ensure_stage(seg_max * sizeof(double));
    if (rc) return rc;
    auto move = [&](double* base, size_t per_slot_window_stride, size_t src_off, size_t n) -> int {
        // base + w*stride + src_off  ->  base + w*stride, n doubles, via the staging buffer
        for (int w = 0; w < v.B; w++) {
            double* dst = base + (size_t)w * per_slot_window_stride;
            vf::launch_shift_copy(dst + src_off, e->stage, (long)n, e->stream);
            vf::launch_shift_copy(e->stage, dst, (long)n, e->stream);
        }
        HIPCHK(hipGetLastError());
        return VF_OK;
    };
    const size_t G = (size_t)v.G, tilesG = G / 64, tilesM = (size_t)v.M / 64, tshift = (size_t)shift / 64;
    // states: [2][16][G] -> per (buf, comp) plane, per window a run of M doubles
    for (int bc = 0; bc < 32; bc++)
        if ((rc = move(v.x + (size_t)bc * G, (size_t)v.M, (size_t)shift, keepk))) return rc;
    // AoSoA arrays: per window tilesM tiles of nf*64 doubles
    struct { double* p; int nf; int bufs; } arrs[] = {{v.imu_in, vf::IMU_IN, 1}, {v.imu_r, vf::IMU_R, 2}, {v.imu_j, JNF, 2},
                                                       {v.btw_in, vf::BTW_IN, 1}, {v.btw_out, vf::BTW_OUT, 2}};
    for (auto& a : arrs)
        for (int bf = 0; bf < a.bufs; bf++) {
            const size_t tile = (size_t)a.nf * 64;
            if ((rc = move(a.p + (size_t)bf * tilesG * tile, tilesM * tile, tshift * tile, (tilesM - tshift) * tile))) return rc;
        }
    // between-factor source indices: move (as raw 4-byte ints, staged through the double buffer) then rebase
    {
        int* stage_i = (int*)e->stage.get();
        for (int w = 0; w < v.B; w++) {
            int* dst = v.btw_a + (size_t)w * v.M;
            HIPCHK(hipMemcpyAsync(stage_i, dst + shift, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(dst, stage_i, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemsetAsync(dst + keepk, 0xff, (size_t)shift * sizeof(int), e->stream));
        }
        vf::launch_shift_btw_a(v.btw_a, v.G, v.M, shift, e->stream);
        HIPCHK(hipGetLastError());
    }
    // ... and their losses with them; the slots freed at the end hold none
    for (int w = 0; w < v.B && v.btw_loss; w++) {
        int* li = v.btw_loss + (size_t)w * v.M;
        double* lk = v.btw_loss_k + (size_t)w * v.M;
        HIPCHK(hipMemcpyAsync(e->stage, li + shift, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(li, e->stage, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemsetAsync(li + keepk, 0, (size_t)shift * sizeof(int), e->stream));
        HIPCHK(hipMemcpyAsync(e->stage, lk + shift, keepk * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(lk, e->stage, keepk * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemsetAsync(lk + keepk, 0, (size_t)shift * sizeof(double), e->stream));
        if (!e->btw_kind) continue;               // ... and their kinds (absolute factors, engine_absolute.inc)
        int* ki = e->btw_kind + (size_t)w * v.M;
        HIPCHK(hipMemcpyAsync(e->stage, ki + shift, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(ki, e->stage, keepk * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemsetAsync(ki + keepk, 0, (size_t)shift * sizeof(int), e->stream));
    }
    // window ranges and prior keys
    std::vector<int> lo(v.B), hi(v.B), pk(v.B);
    HIPCHK(hipMemcpyAsync(pk.data(), v.prior_k, v.B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int w = 0; w < v.B; w++) {
        e->h_lo[w] -= shift; e->h_hi[w] -= shift;
        lo[w] = e->h_lo[w]; hi[w] = e->h_hi[w];
        if (pk[w] >= 0) pk[w] -= shift;
    }
    HIPCHK(hipMemcpyAsync(v.lo, lo.data(), v.B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.hi, hi.data(), v.B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(v.prior_k, pk.data(), v.B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // far between factors: slots move down with the keyframes; one whose older keyframe was reclaimed is gone
    for (int w = 0; w < v.B && v.x_max > 0; w++) {
        if (e->h_xn[w] == 0) continue;
        std::vector<int> a, b, loss;
        std::vector<double> r, lk;
        for (int i = 0; i < e->h_xn[w]; i++) {
            if (e->h_xa[w][i] < shift) continue;
            a.push_back(e->h_xa[w][i] - shift);
            b.push_back(e->h_xb[w][i] - shift);
            r.insert(r.end(), e->h_xrec[w].begin() + (size_t)i * vf::BTW_IN, e->h_xrec[w].begin() + (size_t)(i + 1) * vf::BTW_IN);
            loss.push_back(e->h_xloss[w][i]);
            lk.push_back(e->h_xk[w][i]);
        }
        if (int rc = set_far_list(e, w, (int)a.size(), a.data(), b.data(), r.data(), loss.data(), lk.data())) return rc;
    }
    for (int w = 0; w < v.B && v.x_max > 0; w++) {          // ... and so do the far ends of the linear ones (always inside the window)
        if (e->h_lb[w].empty()) continue;
        for (int& kb : e->h_lb[w]) kb -= shift;
        HIPCHK(hipMemcpyAsync(v.xl_b + (size_t)w * v.x_max, e->h_lb[w].data(), e->h_lb[w].size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return VF_OK;
}

// New engine with more keyframe slots per window, the problem carried over on the device, then swapped into *e (the
// handle the caller holds stays valid).  Inputs and states only: every linearisation, H, g and panel is recomputed by
// the next (cold) solve.
int vf_engine_grow(vf_engine* e, int new_capacity) {
    VF_ENTER(e, Entry::reads);
    if (int rc0 = not_sharded(e, "vf_engine_grow")) return rc0;
    const int M0 = e->v.M, M1 = (new_capacity + 63) / 64 * 64;
    if (M1 <= M0) return fail(VF_ERR_INVALID, "new capacity %d does not exceed the current %d", new_capacity, M0);
    vf_engine_opts o = e->opts;
    o.capacity = M1;
    vf_engine* n = nullptr;
    int rc = create_engine(&o, &e->tune, true, e->stream, &n);     // (on the stream the handle has: the old engine's, handed over below)
    if (rc) return rc;
    const vf::View &a = e->v, &b = n->v;
    const int B = a.B;
    const size_t G0 = (size_t)a.G, G1 = (size_t)b.G;
    // every copy through one of two lambdas that remember the first failure; `copied` waits for them: the new engine is destroyed
    // on any error path
    hipError_t herr = hipStreamSynchronize(e->stream);
    auto cp = [&](void* dst, const void* src, size_t bytes) {
        if (herr == hipSuccess) herr = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, n->stream);
    };
    // a per-window array with `unit` bytes per keyframe slot is B rows of M0 * unit bytes, pitch M0 -> M1 slots: ONE pitched copy
    // per array (36 calls whatever the number of windows; the first version issued 36 copies per window)
    auto cp2 = [&](void* dst, const void* src, size_t unit) {
        if (herr == hipSuccess)
            herr = hipMemcpy2DAsync(dst, (size_t)M1 * unit, src, (size_t)M0 * unit, (size_t)M0 * unit, (size_t)B, hipMemcpyDeviceToDevice, n->stream);
    };
    auto copied = [&]() -> int {
        if (herr == hipSuccess) herr = hipStreamSynchronize(n->stream);
        if (herr == hipSuccess) return VF_OK;
        vf_engine_destroy(n);
        return fail(VF_ERR_DEVICE, "vf_engine_grow: device copy failed: %s", hipGetErrorString(herr));
    };
    for (int pl = 0; pl < 32; pl++) cp2(b.x + (size_t)pl * G1, a.x + (size_t)pl * G0, sizeof(double));     // state planes [2][16][G]
    cp2(b.imu_in, a.imu_in, vf::IMU_IN * sizeof(double));        // AoSoA tiles of 64 slots: whole tiles move (M0, M1 are multiples of 64)
    cp2(b.btw_in, a.btw_in, vf::BTW_IN * sizeof(double));
    cp2(b.btw_a, a.btw_a, sizeof(int));
    cp2(b.delta, a.delta, 15 * sizeof(double));
    struct { void* d; const void* s; size_t bytes; } per_window[] = {
        {b.prior_k, a.prior_k, B * sizeof(int)}, {b.prior_in, a.prior_in, (size_t)B * vf::PRIOR_IN * sizeof(double)},
        {b.mp_on, a.mp_on, B * sizeof(int)}, {b.mp_x, a.mp_x, (size_t)B * 48 * sizeof(double)}, {b.mp_L, a.mp_L, (size_t)B * 729 * sizeof(double)},
        {b.mp_eta, a.mp_eta, (size_t)B * 27 * sizeof(double)}, {b.lo, a.lo, B * sizeof(int)}, {b.hi, a.hi, B * sizeof(int)},
        {b.sel, a.sel, B * sizeof(int)}, {b.lambda, a.lambda, B * sizeof(double)}, {b.cost, a.cost, B * sizeof(double)},
        {b.n_acc, a.n_acc, B * sizeof(int)}, {b.n_rej, a.n_rej, B * sizeof(int)}, {b.n_fail, a.n_fail, B * sizeof(int)},
        {n->lambda0_dev, e->lambda0_dev, B * sizeof(double)}};
    for (auto& c : per_window) cp(c.d, c.s, c.bytes);
    if ((rc = copied())) return rc;
    n->h_lo = e->h_lo;
    n->h_hi = e->h_hi;
    if (e->v.stop_on && (rc = vf_engine_set_convergence(n, e->v.rel_tol, e->v.abs_tol))) { vf_engine_destroy(n); return rc; }
    // (n works on e's stream already -- the caller's, or the handle's own, whose ownership moves to n with the swap below)
    if (e->v.x_max > 0 && e->x_used > 0) {
        // far between factors: the linear ones (they exist on the device only; their arrays do not depend on the capacity) copied,
        // the others re-sent from the host copies
        bool linear = false;
        for (int w = 0; w < e->v.B; w++) linear = linear || !e->h_lb[w].empty();
        if (linear) {
            if ((rc = n->ensure_far(e->x_used))) { vf_engine_destroy(n); return rc; }
            const size_t Bx = (size_t)B * e->x_cap;       // (n is made from e->opts: the same x_cap)
            cp(n->v.xl_n, e->v.xl_n, B * sizeof(int));
            cp(n->v.xl_b, e->v.xl_b, Bx * sizeof(int));
            cp(n->v.xl_U, e->v.xl_U, Bx * 6 * (27 + 6 * (size_t)e->x_cap) * sizeof(double));
            cp(n->v.xl_r0, e->v.xl_r0, Bx * 6 * sizeof(double));
            cp(n->v.xl_bx, e->v.xl_bx, Bx * 7 * sizeof(double));
            if ((rc = copied())) return rc;
            n->attach_far();
            n->h_lb = e->h_lb;
        }
        for (int w = 0; w < e->v.B; w++)
            if (e->h_xn[w] > 0 && (rc = set_far_list(n, w, e->h_xn[w], e->h_xa[w].data(), e->h_xb[w].data(), e->h_xrec[w].data(), e->h_xloss[w].data(), e->h_xk[w].data()))) {
                vf_engine_destroy(n);
                return rc;
            }
        n->recount_far();
    }
    if (e->v.btw_loss) {          // the losses of the band between factors, with their slots
        if ((rc = n->ensure_loss())) { vf_engine_destroy(n); return rc; }
        cp2(n->v.btw_loss, e->v.btw_loss, sizeof(int));
        cp2(n->v.btw_loss_k, e->v.btw_loss_k, sizeof(double));
        if ((rc = copied())) return rc;
    }
    if (e->btw_kind) {            // ... and their kinds (absolute factors)
        if ((rc = n->ensure_kind())) { vf_engine_destroy(n); return rc; }
        cp2(n->btw_kind, e->btw_kind, sizeof(int));
        if ((rc = copied())) return rc;
    }
    // what the solver remembers from solve to solve: the non-monotone rule's damping / excursion state (a whole-history handle
    // grows again and again: each solve after a grow would otherwise restart from lambda0)
    if (e->v.x_best) {
        if ((rc = n->ensure_excursion())) { vf_engine_destroy(n); return rc; }
        cp(n->v.carry, e->v.carry, B * sizeof(int));
        cp(n->v.n_prov, e->v.n_prov, B * sizeof(int));
        cp(n->v.prov, e->v.prov, B * sizeof(int));
        cp(n->v.ref_cost, e->v.ref_cost, B * sizeof(double));
        for (int pl = 0; pl < 16; pl++) cp2(n->v.x_best + (size_t)pl * G1, e->v.x_best + (size_t)pl * G0, sizeof(double));
        if ((rc = copied())) return rc;
    }
    // the arrays change places; the handle -- stream, asynchronous-staging resources, the counters -- stays (EngineHandle)
    e->swap_arrays(*n);
    vf_engine_destroy(n);
    e->mem.grown();
    e->epoch++;
    // the linearisation of the current states is part of the state other entry points rely on (vf_engine_marginalize reads
    // the Jacobians of the oldest keyframe's factors): recompute it in the new buffers
    // (imu_in came over, imu_j did not: the words of the J stream that are the records' own, for every slot -- a record may sit
    // beyond a window's end, preintegrated and not yet appended -- in front of the linearisation that writes the rest)
    vf::launch_fixed_jwords(e->v, 0, e->v.G, e->stream);
    HIPCHK(hipGetLastError());
    bool any = false;
    for (int w = 0; w < e->v.B; w++) any = any || e->h_hi[w] > e->h_lo[w];
    if (any && (rc = vf_engine_linearize(e, 0))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}

int vf_engine_sync(vf_engine* e) {
    VF_ENTER(e, Entry::reads);
    HIPCHK(hipStreamSynchronize(e->stream));
    return VF_OK;
}
