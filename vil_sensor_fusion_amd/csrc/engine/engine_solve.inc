// engine/engine_solve.inc -- the stages of an LM trial, the refined solve, the trial loop (vf_engine_iterate), hipGraph replay.
// A section of vf_engine.hip (the C ABI of the engine: include/vilfusion.h); included from there, inside extern "C", never
// compiled by itself.  struct vf_engine and the helpers every section uses (fail, HIPCHK, Entry) are in vf_engine.hip.
// ------------------------------------------------------------------ stages
// Each stage is a static function that only enqueues -- what vf_engine_iterate's sequence calls, so that a solve does not void
// what it is about to leave behind -- and an entry point of the same name around it, for callers that stage their own trials.
static int linearize(vf_engine* e, int which) {
    which = which ? 1 : 0;
    // time-sharded ranks write the Jacobian of every factor only while the solve is refined (windows longer than
    // refine_min_keyframes, or refine_iterations > 0): otherwise each writes what feeds its own rows, and K1's traffic shrinks
    // with the world size
    e->v.sh_all_jac = e->refine_iters() > 0 ? 1 : 0;
    // a new linearisation of the CURRENT states invalidates H, g and starts a new solve (no window is converged yet)
    if (!which) {
        HIPCHK(hipMemsetAsync(e->v.fresh, 0x01, e->v.B * sizeof(int), e->stream));
        HIPCHK(hipMemsetAsync(e->v.done, 0, e->v.B * sizeof(int), e->stream));
    }
    vf::launch_linearize(e->v, e->btw_kind, which, e->stream);
    if (e->x_used > 0) vf::launch_linearize_extra(e->v, which, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
// What the form of this engine's solves depends on (vf_solve_plan.hpp).  The sweep may not assemble H itself while something in
// the solve reads H and g: the far factors' correction solves, the refined solve's, GTSAM's accept rule (k_model_change).
// (far_veto = false: the plan the same engine without far factors would have -- vf_engine_marginals_ex)
static vf::SolveInputs solve_inputs(const vf_engine* e, bool far_veto = true) {
    return vf::solve_inputs(e->v, e->hybrid && e->v.stop_on, e->act_list != nullptr,
                            (far_veto && e->x_used > 0) || e->refine_iters() > 0 || e->v.min_fidelity > 0.0);
}
static vf::SolvePlan solve_plan(const vf_engine* e) { return vf::solve_plan(solve_inputs(e)); }
static int assemble(vf_engine* e) {
    const vf::K3 k3 = solve_plan(e).k3;
    if (k3 == vf::K3::none) return VF_OK;
    if (k3 == vf::K3::partitioned) {
        vf::launch_assemble_for_partitioned(e->v, e->stream);
        HIPCHK(hipGetLastError());
        return VF_OK;
    }
    vf::launch_assemble(e->v, e->stream);
    if (e->x_used > 0) vf::launch_extra_gradient(e->v, e->stream);   // the far factors' J^T r (their J^T J stays out of the band)
    HIPCHK(hipGetLastError());
    return VF_OK;
}
static int solve(vf_engine* e) {
    if (int rc = not_sharded(e, "vf_engine_solve")) return rc;
    const vf::SolvePlan plan = solve_plan(e);
    auto band_solve = [&](double* gvec, double* delta, const int* skip = nullptr) {      // the engine's K4 form on another right-hand side / increment buffer
        // (skip: windows that take no part -- a refinement's correction solves pass its stop flags, which include the windows
        // the termination rule has finished, so that a window whose corrections have converged costs its later solves nothing)
        const vf::View a = vf::on_buffers(e->v, gvec, delta, skip);
        if (plan.hybrid())      // (the sweeps take their windows from the active list; the partitioned half skips the same windows)
            vf::launch_band_solve(vf::from_active_list(a, e->act_list), vf::on_buffers(e->partitioned_view(), gvec, delta, skip), plan, e->stream);
        else vf::launch_band_solve(a, a, plan, e->stream);
    };
    // (single-window engines with a second stream -- the GraphManager's: the column engine's solve needs H and the far factors'
    // rows, nothing the window's own solve writes, and each of the two is a chain of small launches that leaves most of the part
    // idle: they run side by side, the columns on the second stream)
    bool cols_aside = false;
    if (e->x_used > 0 && e->far_columns && e->stream2 && !e->side_open) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(e->stream, &cap);
        if (cap == hipStreamCaptureStatusNone) {
            const vf::View& c = e->far_columns->v;
            HIPCHK(hipEventRecord(e->ev_fork, e->stream));
            HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
            vf::launch_cols_prepare(e->v, c, 6 * e->x_used, e->stream2);
            vf::launch_partitioned_solve(c, e->stream2);
            HIPCHK(hipEventRecord(e->ev_join, e->stream2));
            cols_aside = true;
        }
    }
    band_solve(e->v.gvec, e->v.delta);
    const double* far_Z = e->x_Z;
    size_t far_zstride = e->x_zstride;
    if (e->x_used > 0) {
        // Far between factors: (H_band + lambda I + U U^T) delta = -g by Woodbury -- the band solver once more per column of
        // U (6 per slot in use; it refactorises every time: a fallback for the rare window with such factors, not a fast
        // path), then one small dense system per window (k_extra_combine).
        if (e->far_columns) {
            // (single-window engines: every column in ONE partitioned solve of the column engine -- same kernels, same bits)
            const vf::View& c = e->far_columns->v;
            if (cols_aside) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
            else {
                vf::launch_cols_prepare(e->v, c, 6 * e->x_used, e->stream);
                vf::launch_partitioned_solve(c, e->stream);
            }
            vf::launch_cols_fail(e->v, c, 6 * e->x_used, e->stream);
            far_Z = c.delta;
            far_zstride = (size_t)c.M * 15;
        } else {
            const size_t gbytes = ((size_t)e->v.G * 15 + 64) * sizeof(double);
            for (int s = 0; s < e->x_used; s++)
                for (int j = 0; j < 6; j++) {
                    HIPCHK(hipMemsetAsync(e->x_gtmp, 0, gbytes, e->stream));
                    vf::launch_extra_rhs(e->v, s, j, e->x_gtmp, e->stream);
                    band_solve(e->x_gtmp, e->x_Z + (size_t)(6 * s + j) * e->x_zstride);
                }
        }
        vf::launch_extra_combine(e->v, far_Z, far_zstride, e->x_used, e->stream);   // (slots beyond x_used are empty in every window)
    }
    if (const int R = e->refine_iters()) {
        // Refined solve (vf_refine.hip): the increment just computed is the start, the factorisation the preconditioner, of
        // conjugate gradients on the normal equations with the operator applied through J -- R correction solves.  With far
        // factors the operator has their rows too (k_far_apply) and the preconditioner is the Woodbury solve above: every
        // correction is one band solve combined with the columns Z that are already there.  (The band factor alone will not
        // do as the preconditioner: against the 1e-10 curvature of a long window's soft modes a loop closure's information is
        // an eigenvalue of 1e14 in M^-1 A, and the band-only start answers the closure's gradient with a step of kilometres.)
        if (int rc = e->ensure_refine()) return rc;
        vf::launch_refine_begin(e->v, e->rq, e->stream);
        for (int it = 0; it < R; it++) {
            band_solve(e->rq.nres, e->rq.z, e->rq.stop);
            if (e->x_used > 0)
                vf::launch_extra_combine(vf::on_buffers(e->v, nullptr, e->rq.z, e->rq.stop), far_Z, far_zstride, e->x_used, e->stream);
            vf::launch_refine_step(e->v, e->rq, e->refine_stop(), e->stream);
            // How many corrections a window needs grows with its length (4 at 1 600 keyframes, 12 at 10 000): after the
            // 4th, 6th, ... the stop flags are read back, and once every window has stopped the rest are not issued
            // (a skipped correction is ~15 empty launches; the read-back costs one stream synchronisation)
            hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(e->stream, &capturing);      // (a caller capturing its own stream: no read-back, every correction is issued)
            if (it >= 1 && it % 2 == 1 && it + 1 < R && capturing == hipStreamCaptureStatusNone) {
                HIPCHK(hipMemcpyAsync(e->rq_stop_host, e->rq.stop, e->v.B * sizeof(int), hipMemcpyDeviceToHost, e->stream));
                HIPCHK(hipStreamSynchronize(e->stream));
                bool live = false;
                for (int w = 0; w < e->v.B && !live; w++) live = e->rq_stop_host[w] == 0;
                if (!live) break;
            }
        }
        vf::launch_refine_end(e->v, e->rq, e->stream);
    }
    HIPCHK(hipGetLastError());
    return VF_OK;
}
// ---- the refined solve on time-sharded engines, staged like the solve itself: after the trial's two collectives
//   vf_engine_refine_begin ; R x { vf_engine_solve_local, <all-gather sep>, vf_engine_solve_global, <all-reduce refine_delta>,
//   vf_engine_refine_step } ; vf_engine_refine_end
// (vf_engine_solve_local / _global work on the correction's right-hand side while a refinement is open)
int vf_engine_refine_count(vf_engine* e, int* iterations) {
    if (!e || !iterations) return fail(VF_ERR_INVALID, "null argument");
    *iterations = e->refine_iters();
    return VF_OK;
}
int vf_engine_refine_begin(vf_engine* e) {
    VF_ENTER(e, Entry::reads);
    e->mem.rewritten();
    if (int rc = e->ensure_refine()) return rc;
    vf::launch_refine_begin(e->v, e->rq, e->stream);
    HIPCHK(hipGetLastError());
    e->refine_open = true;
    return VF_OK;
}
int vf_engine_refine_step(vf_engine* e) {
    Entry entry_(e, Entry::reads);
    if (!e || !e->refine_open) return fail(VF_ERR_INVALID, "no refinement open (vf_engine_refine_begin)");
    vf::launch_refine_step(e->v, e->rq, e->refine_stop(), e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
int vf_engine_refine_end(vf_engine* e) {
    Entry entry_(e, Entry::reads);
    if (!e || !e->refine_open) return fail(VF_ERR_INVALID, "no refinement open (vf_engine_refine_begin)");
    vf::launch_refine_end(e->v, e->rq, e->stream);
    HIPCHK(hipGetLastError());
    e->refine_open = false;
    return VF_OK;
}
// corrections the last refined solve of `window` applied before its stopping rule (or the count) ended it; the ratio of the
// preconditioned residual res . M^-1 res at the end to its first value
int vf_engine_read_refine(vf_engine* e, int window, int* corrections, double* reduction) {
    Entry entry_(e, Entry::reads);
    int rc = check_window(e, window);
    if (rc) return rc;
    int it = 0;
    double rz = 0.0, rz0 = 0.0;
    if (e->rq_ready) {
        HIPCHK(hipMemcpyAsync(&it, e->rq.iters + window, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&rz, e->rq.rz + window, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&rz0, e->rq.rz0 + window, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    if (corrections) *corrections = it;
    if (reduction) *reduction = rz0 > 0.0 ? rz / rz0 : 0.0;
    return VF_OK;
}
static int retract(vf_engine* e) {
    vf::launch_retract(e->v, e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
// non-monotone LM: a failed excursion has put the point it started from back into the current buffer; its factors are
// linearised again (the kernels skip every window whose flag is clear)
static int relinearize_restored(vf_engine* e) {
    vf::launch_linearize(vf::restored_only(e->v), e->btw_kind, 0, e->stream);
    HIPCHK(hipMemsetAsync(e->v.relin, 0, e->v.B * sizeof(int), e->stream));
    return VF_OK;
}
// ... and an excursion still open when a solve's trials run out is undone (vf_engine_iterate does this itself; callers that
// stage their trials -- time-sharded windows -- call it after the last one)
static int close_excursions(vf_engine* e) {
    if (!e->v.x_best) return VF_OK;
    vf::launch_close_excursions(e->v, e->stream);
    if (int rc = relinearize_restored(e)) return rc;
    // the damping of a window that runs the non-monotone rule persists from solve to solve (k_reset_lambda honours the flag):
    // lambda0 = 1e-5 is six orders above the soft eigenvalues of a window long enough to get here, and a solve of five trials
    // that starts there each time spends them all coming down (measured at 8 000 keyframes: 1.5e-5 m from the optimum after
    // four solves of five trials, against 1e-9 after eight trials in one)
    HIPCHK(hipMemsetAsync(e->v.carry, 0x01, e->v.B * sizeof(int), e->stream));
    HIPCHK(hipGetLastError());
    return VF_OK;
}
static int decide(vf_engine* e, int init) {
    e->v.nm_W = e->excursion();
    e->mem.excursions = e->v.nm_W > 0;       // (such trials restore states without their residuals: SolveMemory::residuals_vouched)
    if (e->v.nm_W > 0)
        if (int rc = e->ensure_excursion()) return rc;
    vf::launch_decide(e->v, init ? 1 : 0, e->stream);
    if (e->v.nm_W > 0 && !init)
        if (int rc = relinearize_restored(e)) return rc;
    // what the next K4 launch gates on (and the list its sweeps take their windows from)
    if (e->hybrid && e->v.stop_on) vf::launch_count_active(vf::from_active_list(e->v, e->act_list), e->stream);
    HIPCHK(hipGetLastError());
    return VF_OK;
}
int vf_engine_linearize(vf_engine* e, int which) {
    VF_ENTER(e, Entry::rewrites);
    const int rc = linearize(e, which);
    if (rc == VF_OK && !which) e->mem.residuals_current();      // (every factor, at the current states, into the current buffer)
    return rc;
}
int vf_engine_assemble(vf_engine* e) { VF_ENTER(e, Entry::rewrites); return assemble(e); }
int vf_engine_solve(vf_engine* e) { VF_ENTER(e, Entry::rewrites); return solve(e); }
int vf_engine_retract(vf_engine* e) { VF_ENTER(e, Entry::rewrites); return retract(e); }
int vf_engine_decide(vf_engine* e, int init) { VF_ENTER(e, Entry::rewrites); return decide(e, init); }
int vf_engine_close_excursions(vf_engine* e) { VF_ENTER(e, Entry::reads); return close_excursions(e); }
static int iterate_sequence(vf_engine* e, int iterations) {
    // every solve starts from lambda0, as a fresh LevenbergMarquardtOptimizer would (k_reset_lambda: but on an engine that runs
    // excursions, where close_excursions has marked every window to keep its damping)
    int rc;
    const int slid = e->mem.tail();
    vf::launch_reset_lambda(e->v, e->lambda0_dev, slid ? 1 : 0, e->stream);
    if (slid) {
        // nothing but slides since the last solve: only the appended keyframes' factors and the priors need linearising
        // (no window is converged yet: the flags were cleared with the damping)
        vf::launch_linearize_tail(e->v, e->btw_kind, slid, e->stream);
        HIPCHK(hipGetLastError());
    } else if ((rc = linearize(e, 0))) return rc;
    if ((rc = decide(e, 1))) return rc;
    // One window under the termination rule (the GraphManager's solve): a trial the rule has made unnecessary is eight launches
    // that do nothing (2-4 us each).  Two trials are enqueued blind -- the rule needs two to see convergence, and that is what
    // a steady update takes --; before each further one the window's flag is read (one small synchronisation, paid only by the
    // solves that go on).  The skipped launches would have skipped the window on the device: same bits.
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(e->stream, &capturing);
    // (also with far factors alive, where the staging itself is synchronous: a trial is 21 launches there)
    const bool adaptive = e->v.B == 1 && e->v.stop_on && e->async_on && e->own_stream && e->res_host && capturing == hipStreamCaptureStatusNone;
    // Without excursions to close behind the loop, the read is of the whole result block and comes after the FIRST trial already (a
    // steady update converges in one: what used to follow was an empty trial, 15-21 launches): SolveMemory::result_cached.
    const bool early = adaptive && e->excursion() == 0;
    bool finished = false;
    for (int it = 0; it < iterations; it++) {
        if (early && it >= 1) {
            vf::launch_read_result(e->v, 0, e->h_hi[0] - 1, 0, e->sticky_dev, e->res_host, e->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(e->stream));
            e->mem.sticky_consumed(e->res_host->sticky[0], e->res_host->sticky[1]);        // (handed on with the final result, cached or not)
            e->res_host->sticky[0] = e->res_host->sticky[1] = 0;
            if (e->res_host->pad) { finished = true; break; }
        } else if (adaptive && it >= 2) {
            HIPCHK(hipMemcpyAsync(&e->res_host->pad, e->v.done, sizeof(int), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            if (e->res_host->pad) break;
        }
        if ((rc = assemble(e))) return rc;
        if ((rc = solve(e))) return rc;
        if (e->v.min_fidelity > 0.0) vf::launch_model_change(e->v, e->stream);     // GTSAM's accept rule: what the linearised problem predicts
        if ((rc = retract(e))) return rc;
        if ((rc = linearize(e, 1))) return rc;
        if ((rc = decide(e, 0))) return rc;
    }
    if (iterations > 0 && e->excursion() > 0 && (rc = close_excursions(e))) return rc;
    if (finished) e->mem.result_cached(e->h_hi[0] - 1);
    return VF_OK;
}
// the sequence as plain launches (or under the capture of a caller's stream); on failure the engine is as after any call the
// bookkeeping cannot follow
static int iterate_plain(vf_engine* e, int iterations) {
    const int rc = iterate_sequence(e, iterations);
    if (rc) e->mem.rewritten();
    else e->mem.solve_ended(e->x_used > 0, false);
    return rc;
}
int vf_engine_iterate(vf_engine* e, int iterations) {
    VF_ENTER(e, Entry::reads);
    if (iterations < 0) return fail(VF_ERR_INVALID, "iterations < 0");
    if (int rc0 = not_sharded(e, "vf_engine_iterate")) return rc0;
    // (asynchronous, like the stages: every read-back synchronises the stream)
    if (e->graph_off || !e->own_stream || e->refine_iters() > 0 || e->excursion() > 0) return iterate_plain(e, iterations);
    const int mode = e->mem.tail();      // (baked into the captured sequence: a warm tail of another length is another graph)
    bool replayed = true;                // ... nothing but the replay ran: no host code of the stages
    if (!e->graph_exec || e->graph_iters != iterations || e->graph_epoch != e->epoch || e->graph_mode != mode) {
        e->drop_graph();
        if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            e->graph_off = true;
            return iterate_plain(e, iterations);
        }
        const int rc = iterate_sequence(e, iterations);
        const hipError_t ce = hipStreamEndCapture(e->stream, &e->graph);
        if (rc) { e->drop_graph(); e->mem.rewritten(); return rc; }
        if (ce != hipSuccess || hipGraphInstantiate(&e->graph_exec, e->graph, nullptr, nullptr, 0) != hipSuccess) {
            e->drop_graph();
            e->graph_off = true;          // this runtime cannot capture the sequence: plain launches from now on
            (void)hipGetLastError();
            return iterate_plain(e, iterations);
        }
        e->graph_iters = iterations;
        e->graph_epoch = e->epoch;
        e->graph_mode = mode;
        e->graph_captures++;
        replayed = false;
    }
    HIPCHK(hipGraphLaunch(e->graph_exec, e->stream));
    e->graph_replays++;
    e->mem.solve_ended(e->x_used > 0, replayed);
    return VF_OK;
}
int vf_engine_solve_form(vf_engine* e, int* form) {
    if (!e || !form) return fail(VF_ERR_INVALID, "null argument");
    *form = solve_plan(e).form;
    return VF_OK;
}
int vf_engine_graph_info(vf_engine* e, int* enabled, int* captures, long* replays) {
    if (!e) return fail(VF_ERR_INVALID, "engine is null");
    if (enabled) *enabled = (!e->graph_off && e->own_stream) ? 1 : 0;
    if (captures) *captures = e->graph_captures;
    if (replays) *replays = e->graph_replays;
    return VF_OK;
}
