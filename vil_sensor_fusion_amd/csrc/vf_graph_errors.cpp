// vf_graph_errors.cpp -- vf_get_factor_errors, vf_get_consistency: factor->error(values), graph.error(values) and printErrors for the
// factors of the handle's last solve (include/vilfusion.h).
//
// A translation unit of its own, for the reason vf_graph_scores.cpp states: it calls vf_engine_factor_errors and its readers, which
// the stand-in engine the host tests link vf_graph.cpp against does not have.  It reaches the handle through vf_graph_handle.hpp.
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/vilfusion.h"
#include "vf_graph_handle.hpp"

extern "C" {

void vf_set_last_error_(const char* msg);   // vf_engine.hip

static int eerr(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vf_set_last_error_(buf);
    return code;
}

// the errors of the window as the last solve left it; the caller holds state_mutex.  flags = 0: the residuals the solve left are
// read as they lie (a vf_reserve_node since has written beyond the window's end only); the engine relinearises by itself where it
// cannot vouch for them
static int ensure_errors(vf_graph* g, const double* chi2_threshold6) {
    if (!g->solved_once) return eerr(VF_ERR_INVALID, "no solve yet: there are no factor errors to report");
    if (g->err_valid && !chi2_threshold6) return VF_OK;
    g->err_valid = false;
    if (int rc = vf_engine_factor_errors(g->eng, 0u, chi2_threshold6)) return rc;
    g->err_valid = true;
    return VF_OK;
}

int vf_get_factor_errors(vf_graph* g, uint64_t key0, int n, double* imu_err, double* btw_err, uint64_t* btw_prev_key) {
    if (!g) return eerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (!g->solved_once) return eerr(VF_ERR_INVALID, "no solve yet: there are no factor errors to report");
    if (n < 0 || key0 + (uint64_t)n > g->solved_key + 1)
        return eerr(VF_ERR_BAD_KEY, "keys [%llu, %llu) not solved yet (last solved key %llu)", (unsigned long long)key0, (unsigned long long)(key0 + n),
                    (unsigned long long)g->solved_key);
    if (key0 < oldest_key(g)) return eerr(VF_ERR_BAD_KEY, "key %llu has left the window (oldest key %llu)", (unsigned long long)key0, (unsigned long long)oldest_key(g));
    if (int rc = ensure_errors(g, nullptr)) return rc;
    std::vector<int32_t> a(btw_prev_key ? (size_t)n : 0);
    if (int rc = vf_engine_read_factor_errors(g->eng, 0, slot_of(g, key0), n, imu_err, btw_err, btw_prev_key ? a.data() : nullptr)) return rc;
    // (an absolute factor sits in its key's slot as one from the key before: it is reported as a factor on ONE key, prev == key)
    std::vector<int32_t> kind(a.size());
    if (!a.empty())
        if (int rc = vf_engine_get_absolute(g->eng, 0, slot_of(g, key0), n, kind.data())) return rc;
    for (size_t i = 0; i < a.size(); i++)
        btw_prev_key[i] = a[i] < 0 ? UINT64_MAX : kind[i] != VF_ABSOLUTE_NONE ? key0 + (uint64_t)i : g->key_base + (uint64_t)a[i];
    return VF_OK;
}

int vf_get_far_factors(vf_graph* g, int* n, uint64_t* prev_key, uint64_t* cur_key, int* loss, double* k, double* err) {
    if (!g || !n) return eerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (int rc = ensure_errors(g, nullptr)) return rc;
    int cnt = 0;
    int32_t a[VF_MAX_FAR_LIMIT], b[VF_MAX_FAR_LIMIT], li[VF_MAX_FAR_LIMIT];
    double kk[VF_MAX_FAR_LIMIT], fe[VF_MAX_FAR_LIMIT], fl[VF_MAX_FAR_LIMIT];
    if (int rc = vf_engine_get_extra_between(g->eng, 0, &cnt, a, b, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (int rc = vf_engine_get_extra_between_loss(g->eng, 0, li, kk)) return rc;
    if (int rc = vf_engine_read_far_errors(g->eng, 0, fe, fl)) return rc;
    *n = cnt;
    for (int i = 0; i < cnt; i++) {
        if (prev_key) prev_key[i] = g->key_base + (uint64_t)a[i];
        if (cur_key) cur_key[i] = g->key_base + (uint64_t)b[i];
        if (loss) loss[i] = li[i];
        if (k) k[i] = kk[i];
        if (err) err[i] = fe[i];
    }
    return VF_OK;
}

int vf_get_consistency(vf_graph* g, const double* chi2_threshold6, vf_consistency* out) {
    if (!g || !out) return eerr(VF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(g->state_mutex);
    if (int rc = ensure_errors(g, chi2_threshold6)) return rc;
    return vf_engine_read_consistency(g->eng, 0, out);
}

}  // extern "C"
