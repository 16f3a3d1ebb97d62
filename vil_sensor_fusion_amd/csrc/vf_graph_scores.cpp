// vf_graph_scores.cpp -- vf_get_degeneracy_scores: the degeneracy scores of the handle's own estimate (include/vilfusion.h).
//
// A translation unit of its own: it calls vf_engine_marginal_scores / vf_engine_read_marginal_scores, which the stand-in engine
// the host tests link vf_graph.cpp against does not have.  It reaches the handle through vf_graph_handle.hpp.
#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int serr(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

int vf_get_degeneracy_scores(vf_graph* g, int source, int metric, unsigned subset_mask, uint64_t key0, int n, double* out) {
    if (!g || !out) return serr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (!g->solved_once) return serr(VF_ERR_INVALID, "no solve yet: there are no covariances to score");
    if (n < 0 || key0 + (uint64_t)n > g->solved_key + 1)
        return serr(VF_ERR_BAD_KEY, "keys [%llu, %llu) not solved yet (last solved key %llu)", (unsigned long long)key0, (unsigned long long)(key0 + n),
                    (unsigned long long)g->solved_key);
    if (key0 < oldest_key(g)) return serr(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)key0, (unsigned long long)oldest_key(g));
    if (!g->cov_valid || !g->cov_pose) {
        // (far_covariance: as vf_get_marginal_covariance; a call of that one since the solve has left covariances without the
        // nav_msgs records: they are computed again with them, the same bits)
        if (int rc = vf_engine_marginals_ex(g->eng, VF_MARGINALS_POSE | (g->opts.far_covariance ? VF_MARGINALS_FAR : 0u))) return rc;
        g->cov_valid = g->cov_pose = true;
        g->cov_tail = false;
    }
    if (int rc = vf_engine_marginal_scores(g->eng, source, metric, subset_mask)) return rc;
    return vf_engine_read_marginal_scores(g->eng, 0, slot_of(g, key0), n, out);
}

}  // extern "C"
