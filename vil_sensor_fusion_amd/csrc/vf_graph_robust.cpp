// vf_graph_robust.cpp -- vf_add_between_robust and vf_graph_get_staged_loss: between factors with a robust loss on the handle
// (include/vilfusion.h).
//
// A translation unit of its own, beside vf_graph_gate.cpp and for its reason: it names vf_engine_set_between_loss,
// vf_engine_set_extra_between_robust and vf_engine_get_extra_between_loss, which the stand-in engine the host tests link vf_graph.cpp
// against does not have.  vf_graph.cpp's staging steps reach those calls through pointers in the handle, which the first robust
// factor sets here; while they are null nothing is called.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int robust_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

int vf_add_between_robust(vf_graph* g, uint64_t prev_key, uint64_t cur_key, const double q_wxyz[4], const double t[3], const double cov36[36],
                          int loss, double k) {
    if (loss < VF_LOSS_NONE || loss > VF_LOSS_GEMAN_MCCLURE) return robust_err(VF_ERR_INVALID, "vf_add_between_robust: unknown loss id %d", loss);
    if (loss != VF_LOSS_NONE && !(k > 0.0 && std::isfinite(k)))
        return robust_err(VF_ERR_INVALID, "vf_add_between_robust: the parameter k must be finite and > 0 (got %g)", k);
    // (band factors: the loss behind the record; far factors, vf_set_robust_far: the loss with the list, and back with it)
    static const vf_robust_calls calls{&vf_engine_set_between_loss, &vf_engine_set_extra_between_robust, &vf_engine_get_extra_between_loss};
    return vf_add_between_(g, prev_key, cur_key, q_wxyz, t, cov36, loss, k, loss == VF_LOSS_NONE ? nullptr : &calls);
}

int vf_set_robust_far(vf_graph* g, int on) {
    if (!g) return robust_err(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    g->robust_far = on != 0;
    return VF_OK;
}

int vf_graph_get_staged_loss(vf_graph* g, int index, int* loss, double* k) {
    if (!g) return robust_err(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->graph_mutex);
    const int np = g->priors_staged ? 3 : 0;
    if (index < 0 || index >= np + (int)g->staged_log.size()) return robust_err(VF_ERR_BAD_KEY, "staged factor %d of %d", index, np + (int)g->staged_log.size());
    const bool between = index >= np;
    if (loss) *loss = between ? g->staged_log[(size_t)(index - np)].loss : VF_LOSS_NONE;
    if (k) *k = between ? g->staged_log[(size_t)(index - np)].loss_k : 0.0;
    return VF_OK;
}

}  // extern "C"
