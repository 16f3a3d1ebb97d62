// vf_graph_predict.cpp -- vf_predict_state: the handle's estimate at IMU rate, between two solves (include/vilfusion.h).
//
// A translation unit of its own: it calls vf_engine_propagate_tail / vf_engine_read_propagated, which the stand-in engine the host
// tests link vf_graph.cpp against does not have.  It reaches the handle through vf_graph_handle.hpp.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"
#include "vf_predict_steps.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int perr(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

// Locks: graph -> buffer (released) -> state, as vf_reserve_node.  Never from inside a callback (they run inside state_mutex).
int vf_predict_state(vf_graph* g, double time, double q[4], double t[3], double v[3], double bias[6], double cov225[225]) {
    if (!g) return perr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    if (g->current_key < 1) return perr(VF_ERR_INVALID, "vf_predict_state: no solve yet: there is no state to predict from");
    const double start = g->last_pose_time;
    if (time < start) return perr(VF_ERR_INVALID, "vf_predict_state(%.6f): precedes the last reserved key's time %.6f", time, start);
    // the steps of every queued, not yet solved factor, then what vf_reserve_node(time) would cut now
    std::vector<double> steps;
    for (const auto& p : g->imu_queue) {
        if (!p.record.empty())
            return perr(VF_ERR_INVALID, "vf_predict_state: the queued factor of key %llu is a ready-made record (vf_add_imu_factor): it has no steps to integrate",
                        (unsigned long long)p.key);
        steps.insert(steps.end(), p.steps.begin(), p.steps.end());
    }
    const uint64_t queued = g->imu_queue.size(), last_key = g->current_key;
    if (time > start) {       // (no time since the last key: nothing is cut, not even the rule's interpolated step of zero length)
        std::lock_guard<std::mutex> bl(g->buffer_mutex);
        vf_predict_steps(g->buffer, start, time, steps);
    }
    std::lock_guard<std::mutex> sl(g->state_mutex);
    if (!g->solved_once) return perr(VF_ERR_INVALID, "vf_predict_state: no solve yet: there is no state to predict from");
    if (g->solved_key + queued != last_key)
        return perr(VF_ERR_INVALID, "vf_predict_state: the last solve failed and its factors are being queued again: solve first");
    unsigned flags = (g->opts.reference_compat && g->solved_key > 0) ? VF_PROPAGATE_FROM_ESTIMATE : 0u;
    if (cov225) {
        if (g->solved_key < oldest_key(g))
            return perr(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)g->solved_key, (unsigned long long)oldest_key(g));
        if (!g->cov_valid) {
            // (as vf_get_marginal_covariance: far_covariance takes far factors alive into account; without it they are refused)
            if (int rc = g->opts.far_covariance ? vf_engine_marginals_ex(g->eng, VF_MARGINALS_FAR) : vf_engine_marginals(g->eng)) return rc;
            g->cov_valid = true;
            g->cov_pose = g->cov_tail = false;
        }
        flags |= VF_PROPAGATE_COVARIANCE;
    }
    const int32_t off[2] = {0, (int32_t)(steps.size() / 7)};
    if (int rc = vf_engine_propagate_tail(g->eng, off, steps.data(), &g->imu, flags)) return rc;
    double st[16];
    if (int rc = vf_engine_read_propagated(g->eng, 0, st, cov225)) return rc;
    if (q) memcpy(q, st, sizeof(double) * 4);
    if (t) memcpy(t, st + 4, sizeof(double) * 3);
    if (v) memcpy(v, st + 7, sizeof(double) * 3);
    if (bias) memcpy(bias, st + 10, sizeof(double) * 6);
    return VF_OK;
}

}  // extern "C"
