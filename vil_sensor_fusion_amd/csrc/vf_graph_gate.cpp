// vf_graph_gate.cpp -- vf_gate_between: the innovation test of an odometry increment before vf_add_between takes it; vf_gate_closure:
// the same test of a loop closure between two solved keys (include/vilfusion.h).
//
// A translation unit of its own, beside vf_graph_predict.cpp and for its reason: it calls vf_engine_gate_tail / vf_engine_read_gate
// and vf_engine_gate_closures / vf_engine_read_closure_gate, which the stand-in engine the host tests link vf_graph.cpp against does not have.  It reaches the handle through
// vf_graph_handle.hpp.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int gate_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

// Locks: graph -> state, as vf_predict_state (the IMU buffer is not read: the steps are those of the queued factors).  Never from
// inside a callback (they run inside state_mutex).  Nothing is consumed or staged: the queue, the staged factors and the buffer are
// as they were, and the engine call writes a buffer of its own.  The one thing that may be computed on the way is the covariances,
// which leave the next solve the bits it would have had (vf_engine_marginals_ex).
int vf_gate_between(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q[4], const double t[3], const double cov36[36],
                    double chi2_threshold, vf_gate_result* out) {
    if (!g || !q || !t || !cov36 || !out) return gate_err(VF_ERR_INVALID, "null argument");
    double rec[VF_BTW_RECORD];
    if (int rc = vf_between_record_(q, t, cov36, rec)) return rc;
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (g->current_key < 1) return gate_err(VF_ERR_INVALID, "vf_gate_between: no solve yet: there is no state to predict from");
    if (prev_key >= cur_key || cur_key > g->current_key)
        return gate_err(VF_ERR_BAD_KEY, "between factor keys (%llu, %llu) not reserved in order", (unsigned long long)prev_key, (unsigned long long)cur_key);
    // the steps of the queued, not yet solved factors up to cur_key, concatenated as vf_predict_state does
    std::vector<double> steps;
    for (const auto& p : g->imu_queue) {
        if (p.key > cur_key) break;
        if (!p.record.empty())
            return gate_err(VF_ERR_INVALID, "vf_gate_between: the queued factor of key %llu is a ready-made record (vf_add_imu_factor): it has no steps to integrate",
                            (unsigned long long)p.key);
        steps.insert(steps.end(), p.steps.begin(), p.steps.end());
    }
    const uint64_t queued = g->imu_queue.size(), last_key = g->current_key;
    std::lock_guard<std::mutex> sl(g->state_mutex);
    if (!g->solved_once) return gate_err(VF_ERR_INVALID, "vf_gate_between: no solve yet: there is no state to predict from");
    if (g->solved_key + queued != last_key)
        return gate_err(VF_ERR_INVALID, "vf_gate_between: the last solve failed and its factors are being queued again: solve first");
    if (cur_key < g->solved_key)
        return gate_err(VF_ERR_BAD_KEY, "vf_gate_between: key %llu is solved already (last solved key %llu): the gate tests a factor that ends at or beyond it",
                        (unsigned long long)cur_key, (unsigned long long)g->solved_key);
    if (g->solved_key < oldest_key(g))
        return gate_err(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)g->solved_key, (unsigned long long)oldest_key(g));
    // reach: the last solved key or the one before it, still in the window; anything else is a status the kernel gives
    const int last_slot = slot_of(g, g->solved_key);
    int32_t a = prev_key > g->solved_key ? last_slot + 1 : (prev_key < oldest_key(g) ? -2 : slot_of(g, prev_key));
    if (!g->cov_valid) {
        const bool far_alive = g->far_on_device || g->far_linear.load() > 0;
        if (!far_alive) {
            if (int rc = vf_engine_marginals_ex(g->eng, VF_MARGINALS_TAIL)) return rc;
            g->cov_tail = true;
        } else {
            // (as vf_predict_state: far_covariance takes far factors alive into account; without it they are refused)
            if (int rc = g->opts.far_covariance ? vf_engine_marginals_ex(g->eng, VF_MARGINALS_FAR) : vf_engine_marginals(g->eng)) return rc;
            g->cov_tail = false;
        }
        g->cov_valid = true;
        g->cov_pose = false;
    }
    const unsigned flags = (g->opts.reference_compat && g->solved_key > 0) ? VF_GATE_FROM_ESTIMATE : 0u;
    const int32_t off[2] = {0, (int32_t)(steps.size() / 7)};
    if (int rc = vf_engine_gate_tail(g->eng, off, steps.data(), &g->imu, &a, rec, chi2_threshold, flags)) return rc;
    return vf_engine_read_gate(g->eng, 0, out);
}

// Locks and refusals as vf_gate_between.  Nothing is consumed or staged, and no covariance the handle keeps is touched: the engine
// call factors the window itself and writes buffers of its own (vf_engine_gate_closures), leaving the next solve the bits it would
// have had.  Far factors alive are part of the covariance whatever vf_graph_opts.far_covariance says.
int vf_gate_closure(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q[4], const double t[3], const double cov36[36],
                    double chi2_threshold, vf_closure_gate_result* out, double* joint_cov144) {
    if (!g || !q || !t || !cov36 || !out) return gate_err(VF_ERR_INVALID, "null argument");
    double rec[VF_BTW_RECORD];
    if (int rc = vf_between_record_(q, t, cov36, rec)) return rc;
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (g->current_key < 1) return gate_err(VF_ERR_INVALID, "vf_gate_closure: no solve yet: there is no window to test against");
    if (prev_key >= cur_key || cur_key > g->current_key)
        return gate_err(VF_ERR_BAD_KEY, "between factor keys (%llu, %llu) not reserved in order", (unsigned long long)prev_key, (unsigned long long)cur_key);
    const uint64_t queued = g->imu_queue.size(), last_key = g->current_key;
    std::lock_guard<std::mutex> sl(g->state_mutex);
    if (!g->solved_once) return gate_err(VF_ERR_INVALID, "vf_gate_closure: no solve yet: there is no window to test against");
    if (g->solved_key + queued != last_key)
        return gate_err(VF_ERR_INVALID, "vf_gate_closure: the last solve failed and its factors are being queued again: solve first");
    // both keys solved and still in the window; anything else is a status, which the engine gives for slots outside [lo, hi)
    const int32_t w = 0;
    const bool reach = cur_key <= g->solved_key && prev_key >= oldest_key(g);
    const int32_t a = reach ? slot_of(g, prev_key) : -2, b = reach ? slot_of(g, cur_key) : -3;
    const unsigned flags = (g->opts.reference_compat && g->solved_key > 0) ? VF_GATE_FROM_ESTIMATE : 0u;      // (as vf_gate_between)
    if (int rc = vf_engine_gate_closures_ex(g->eng, 1, &w, &a, &b, rec, chi2_threshold, flags)) return rc;
    return vf_engine_read_closure_gate(g->eng, 0, out, joint_cov144);
}

}  // extern "C"
