// vf_graph_absolute.cpp -- vf_add_absolute_pose, vf_add_absolute_position and vf_get_absolute_factors: absolute factors on the handle
// (include/vilfusion.h "Absolute pose and position factors on keyframes").
//
// A translation unit of its own, beside vf_graph_robust.cpp and for its reason: it names vf_engine_set_absolute,
// vf_engine_get_absolute and vf_absolute_position_record, which the stand-in engine the host tests link vf_graph.cpp against does
// not have.  vf_graph.cpp's staging step reaches vf_engine_set_absolute through a pointer in the handle, which the first absolute
// factor sets here; while it is null nothing is called.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int abs_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

static int check_loss(const char* who, int loss, double k) {
    if (loss < VF_LOSS_NONE || loss > VF_LOSS_GEMAN_MCCLURE) return abs_err(VF_ERR_INVALID, "%s: unknown loss id %d", who, loss);
    if (loss != VF_LOSS_NONE && !(k > 0.0 && std::isfinite(k))) return abs_err(VF_ERR_INVALID, "%s: the parameter k must be finite and > 0 (got %g)", who, k);
    return VF_OK;
}

static int add(vf_graph* g, uint64_t key, int kind, const double* rec, const StagedFactor& shown, int loss, double k) {
    static const vf_robust_calls calls{&vf_engine_set_between_loss, &vf_engine_set_extra_between_robust, &vf_engine_get_extra_between_loss};
    return vf_add_absolute_(g, key, kind, rec, &shown, loss, k, &vf_engine_set_absolute, loss == VF_LOSS_NONE ? nullptr : &calls);
}

int vf_add_absolute_pose(vf_graph* g, uint64_t key, const double q_wxyz[4], const double t[3], const double cov36[36], int loss, double k) {
    if (!g || !q_wxyz || !t || !cov36) return abs_err(VF_ERR_INVALID, "null argument");
    if (int rc = check_loss("vf_add_absolute_pose", loss, k)) return rc;
    double rec[VF_BTW_RECORD];
    if (int rc = vf_between_record_(q_wxyz, t, cov36, rec)) return rc;     // (the record of a pose factor IS a between record: Z and R)
    StagedFactor shown{};
    memcpy(shown.q, rec, sizeof(shown.q));
    memcpy(shown.t, t, sizeof(shown.t));
    memcpy(shown.cov, cov36, sizeof(shown.cov));
    return add(g, key, VF_ABSOLUTE_POSE, rec, shown, loss, k);
}

int vf_add_absolute_position(vf_graph* g, uint64_t key, const double p[3], const double cov9[9], int loss, double k) {
    if (!g || !p || !cov9) return abs_err(VF_ERR_INVALID, "null argument");
    if (int rc = check_loss("vf_add_absolute_position", loss, k)) return rc;
    double rec[VF_BTW_RECORD];
    if (int rc = vf_absolute_position_record(p, cov9, rec)) return rc;
    StagedFactor shown{};
    shown.q[0] = 1.0;
    memcpy(shown.t, p, sizeof(shown.t));
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) shown.cov[(3 + i) * 6 + 3 + j] = cov9[i * 3 + j];      // the translation block
    return add(g, key, VF_ABSOLUTE_POSITION, rec, shown, loss, k);
}

int vf_get_absolute_factors(vf_graph* g, uint64_t key0, int n, int32_t* kind) {
    if (!g || (n > 0 && !kind)) return abs_err(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (n < 0 || key0 + (uint64_t)n > g->solved_key + 1)
        return abs_err(VF_ERR_BAD_KEY, "keys [%llu, %llu) not solved yet (last solved key %llu)", (unsigned long long)key0, (unsigned long long)(key0 + n),
                       (unsigned long long)g->solved_key);
    if (key0 < oldest_key(g)) return abs_err(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)key0, (unsigned long long)oldest_key(g));
    return vf_engine_get_absolute(g->eng, 0, slot_of(g, key0), n, kind);
}

}  // extern "C"
