// Host-logic test double for the engine half of libvilfusion (tests only; never shipped): every vf_engine_* entry point
// vf_graph.cpp calls, with no device behind it, so that the GraphManager bookkeeping (queues, give-back, the two-lock
// discipline of GraphManager.h:103-104) can be driven on a CPU and under ThreadSanitizer.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define VF_NO_SIZED_DEFAULTS      /* this file DEFINES the functions the header's macros of the same name would shadow */
#include "../../include/vilfusion.h"

// (the far list is kept the way the real engine keeps it: replaced by vf_engine_set_extra_between, transported to the next
// keyframe when its older keyframe is dropped, shifted by a compaction)
struct FarEntry { int a, b; double rec[VF_BTW_RECORD]; };
struct vf_engine { int lo = 0, hi = 0; std::vector<FarEntry> far; };
static thread_local std::string g_err;
std::atomic<int> fake_fail_preintegrate{0};   // != 0: vf_engine_preintegrate fails (the solve gives its queues back)
std::atomic<long> fake_iterates{0};
// what the last vf_engine_set_between / vf_engine_set_extra_between calls carried (host-logic tests of the far-factor routing)
std::atomic<int> fake_band_n{-1}, fake_extra_n{-1}, fake_extra_calls{0}, fake_extra_a0{-1}, fake_extra_b0{-1};
// what vf_engine_read_result reports next to the state: the sticky flags of the staging kernels and the failed LM trials
std::atomic<int> fake_result_flags{0}, fake_result_fails{0};
// The call log (tests/native/graph_trace.cpp; single-threaded use only).  Off by default.  On: every entry point appends one line
// to fake_log -- its name, its scalar arguments, the contents of its input arrays (for records their first doubles), which of its
// outputs were asked for.  No pointers, no times: two builds of vf_graph.cpp that make the same calls leave the same text.
std::atomic<bool> fake_log_on{false};
std::string fake_log;

static void logf(const char* fmt, ...) {
    if (!fake_log_on.load()) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fake_log += buf;
}
static void log_ints(const char* name, const int32_t* v, int n) {
    logf(" %s=[", name);
    for (int i = 0; i < n; i++) logf(i ? " %d" : "%d", v[i]);
    logf("]");
}
// n records of `stride` doubles: the first `first` of each
static void log_recs(const char* name, const double* v, int n, int stride, int first) {
    logf(" %s=[", name);
    for (int i = 0; i < n; i++) {
        logf(i ? " |" : "");
        for (int j = 0; j < first && j < stride; j++) logf(" %.17g", v[(size_t)i * stride + j]);
    }
    logf(" ]");
}

extern "C" {
const char* vf_last_error(void) { return g_err.c_str(); }
void vf_set_last_error_(const char* m) { g_err = m ? m : ""; }
void vf_engine_default_opts(vf_engine_opts* o) {
    logf("default_opts\n");
    memset(o, 0, sizeof(*o)); o->struct_size = (uint32_t)sizeof(*o); o->windows = 1; o->capacity = 1088; o->bandwidth = 3;
}
int vf_engine_incremental_info(vf_engine*, int w, long* u, long* f, int* a, int* b) {
    logf("incremental_info w=%d\n", w);
    if (u) *u = 0; if (f) *f = 0; if (a) *a = -1; if (b) *b = -1; return VF_OK;
}
int vf_engine_create(const vf_engine_opts* o, vf_engine** out) {
    logf("create windows=%d capacity=%d device=%d cold_start=%d min_model_fidelity=%.17g max_far_factors=%d incremental=%d wildfire=%.17g refine_iterations=%d lm_excursion=%d\n",
         o->windows, o->capacity, o->device, o->cold_start, o->min_model_fidelity, o->max_far_factors, o->incremental, o->wildfire, o->refine_iterations, o->lm_excursion);
    *out = new vf_engine(); return VF_OK;
}
void vf_engine_destroy(vf_engine* e) { logf("destroy\n"); delete e; }
int vf_engine_set_states(vf_engine*, int w, int k0, int n, const double* s) { logf("set_states w=%d k0=%d n=%d", w, k0, n); log_recs("state", s, n, 16, 16); logf("\n"); return VF_OK; }
int vf_engine_set_prior(vf_engine*, int w, int k, const double* rec) { logf("set_prior w=%d k=%d", w, k); log_recs("rec", rec, 1, VF_PRIOR_RECORD, VF_PRIOR_RECORD); logf("\n"); return VF_OK; }
int vf_engine_set_range(vf_engine* e, int w, int lo, int hi) { logf("set_range w=%d lo=%d hi=%d\n", w, lo, hi); e->lo = lo; e->hi = hi; return VF_OK; }
int vf_engine_set_convergence(vf_engine*, double r, double a) { logf("set_convergence rel=%.17g abs=%.17g\n", r, a); return VF_OK; }
int vf_engine_set_imu(vf_engine*, int w, int k0, int n, const double* rec) { logf("set_imu w=%d k0=%d n=%d", w, k0, n); log_recs("rec", rec, n, VF_IMU_RECORD, 4); logf("\n"); return VF_OK; }
int vf_engine_preintegrate(vf_engine*, int w, int k0, int n, const int32_t* off, const double* steps, const double* bias, const vf_imu_params* p) {
    logf("preintegrate w=%d k0=%d n=%d", w, k0, n);
    log_ints("off", off, n + 1);
    log_recs("steps", steps, off[n], 7, 2);
    log_recs("bias", bias, n, 6, 6);
    logf(" imu=%.17g,%.17g,%.17g,%.17g,%.17g,%.17g fail=%d\n", p->acc_cov, p->gyro_cov, p->integration_cov, p->bias_acc_cov, p->bias_omega_cov, p->bias_acc_omega_int,
         fake_fail_preintegrate.load());
    if (fake_fail_preintegrate.load()) { g_err = "fake: preintegration refused"; return VF_ERR_DEVICE; }
    return VF_OK;
}
int vf_engine_predict(vf_engine*, int w, int k0, int n) { logf("predict w=%d k0=%d n=%d\n", w, k0, n); return VF_OK; }
int vf_engine_predict_from_estimate(vf_engine*, int w, int k0, int n) { logf("predict_from_estimate w=%d k0=%d n=%d\n", w, k0, n); return VF_OK; }
int vf_engine_set_between(vf_engine*, int w, int n, const int32_t* a, const int32_t* b, const double* rec) {
    logf("set_between w=%d n=%d", w, n); log_ints("a", a, n); log_ints("b", b, n); log_recs("rec", rec, n, VF_BTW_RECORD, 8); logf("\n");
    fake_band_n = n; return VF_OK;
}
int vf_engine_set_extra_between(vf_engine* e, int w, int n, const int32_t* a, const int32_t* b, const double* rec) {
    logf("set_extra_between w=%d n=%d", w, n); log_ints("a", a, n); log_ints("b", b, n); log_recs("rec", rec, n, VF_BTW_RECORD, 8); logf("\n");
    e->far.clear();
    for (int i = 0; i < n; i++) { FarEntry f; f.a = a[i]; f.b = b[i]; memcpy(f.rec, rec + (size_t)i * VF_BTW_RECORD, sizeof(f.rec)); e->far.push_back(f); }
    fake_extra_n = n;
    fake_extra_calls++;
    fake_extra_a0 = n ? a[0] : -1;
    fake_extra_b0 = n ? b[0] : -1;
    return VF_OK;
}
int vf_engine_marginalize(vf_engine*) { logf("marginalize\n"); return VF_OK; }
int vf_engine_refine_count(vf_engine*, int* n) { logf("refine_count\n"); if (n) *n = 0; return VF_OK; }
int vf_engine_read_excursions(vf_engine*, int w, int* a, int* b) { logf("read_excursions w=%d\n", w); if (a) *a = 0; if (b) *b = 0; return VF_OK; }
int vf_engine_drop_oldest(vf_engine* e) {
    logf("drop_oldest\n");
    std::vector<FarEntry> keep;
    for (auto f : e->far) {
        if (f.a == e->lo) { if (f.b - f.a <= 3) continue; f.a++; }      // (short enough for the marginal prior: absorbed)
        keep.push_back(f);
    }
    e->far.swap(keep);
    e->lo++;
    return VF_OK;
}
int vf_engine_compact(vf_engine* e, int shift) {
    logf("compact shift=%d\n", shift);
    for (auto& f : e->far) { f.a -= shift; f.b -= shift; }
    e->lo -= shift; e->hi -= shift;
    return VF_OK;
}
int vf_engine_get_extra_between(vf_engine* e, int w, int* n, int32_t* a, int32_t* b, double* rec, long* tr, long* en, long* ab) {
    logf("get_extra_between w=%d wants n=%d a=%d b=%d rec=%d transported=%d ended=%d absorbed=%d -> %d\n", w, n != nullptr, a != nullptr, b != nullptr, rec != nullptr,
         tr != nullptr, en != nullptr, ab != nullptr, (int)e->far.size());
    if (n) *n = (int)e->far.size();
    for (size_t i = 0; i < e->far.size(); i++) {
        if (a) a[i] = e->far[i].a;
        if (b) b[i] = e->far[i].b;
        if (rec) memcpy(rec + i * VF_BTW_RECORD, e->far[i].rec, sizeof(e->far[i].rec));
    }
    if (tr) *tr = 0;
    if (en) *en = 0;
    if (ab) *ab = 0;
    return VF_OK;
}
int vf_engine_get_linear_far(vf_engine*, int w, int* n, int32_t* far_end) { logf("get_linear_far w=%d wants n=%d far_end=%d\n", w, n != nullptr, far_end != nullptr); if (n) *n = 0; return VF_OK; }
int vf_engine_grow(vf_engine*, int cap) { logf("grow capacity=%d\n", cap); return VF_OK; }
int vf_engine_isam_step(vf_engine*, double thr) { logf("isam_step relin_threshold=%.17g\n", thr); return VF_OK; }
int vf_engine_iterate(vf_engine*, int it) { logf("iterate iterations=%d\n", it); fake_iterates++; return VF_OK; }
int vf_engine_read_lm(vf_engine*, int w, double* c, double* l, int* a, int* r, int* f) {
    logf("read_lm w=%d wants cost=%d lambda=%d accepted=%d rejected=%d failures=%d\n", w, c != nullptr, l != nullptr, a != nullptr, r != nullptr, f != nullptr);
    if (c) *c = 0; if (l) *l = 0; if (a) *a = 0; if (r) *r = 0; if (f) *f = 0;
    return VF_OK;
}
static int fill_state(int n, double* s) { for (int i = 0; i < n; i++) { memset(s + 16 * i, 0, 16 * sizeof(double)); s[16 * i] = 1.0; } return VF_OK; }
int vf_engine_get_states(vf_engine*, int w, int k0, int n, double* s) { logf("get_states w=%d k0=%d n=%d\n", w, k0, n); return fill_state(n, s); }
int vf_engine_get_estimate(vf_engine*, int w, int k0, int n, double* s) { logf("get_estimate w=%d k0=%d n=%d\n", w, k0, n); return fill_state(n, s); }
int vf_engine_set_async(vf_engine*, int on) { logf("set_async on=%d\n", on); return VF_OK; }
int vf_engine_marginalize_ahead(vf_engine*) { logf("marginalize_ahead\n"); return VF_OK; }
// (the state it reports carries the slot it was asked for as its x position, so that a caller's copy shows which solve wrote it)
int vf_engine_read_result(vf_engine*, int w, int slot, int estimate, double* s, double* c, int* a, int* r, int* f, int* flags) {
    logf("read_result w=%d slot=%d estimate=%d wants state=%d cost=%d accepted=%d rejected=%d failures=%d flags=%d -> failures %d flags %d\n", w, slot, estimate, s != nullptr,
         c != nullptr, a != nullptr, r != nullptr, f != nullptr, flags != nullptr, fake_result_fails.load(), fake_result_flags.load());
    if (c) *c = 0.0;
    if (a) *a = 0;
    if (r) *r = 0;
    if (f) *f = fake_result_fails.load();
    if (flags) *flags = fake_result_flags.load();
    if (s) { fill_state(1, s); s[4] = (double)slot; }
    return VF_OK;
}
int vf_engine_get_imu(vf_engine*, int w, int k0, int n, double* r) { logf("get_imu w=%d k0=%d n=%d\n", w, k0, n); memset(r, 0, sizeof(double) * VF_IMU_RECORD * n); return VF_OK; }
int vf_engine_marginals(vf_engine*) { logf("marginals\n"); return VF_OK; }
int vf_engine_marginals_ex(vf_engine*, unsigned flags) { logf("marginals_ex flags=%u\n", flags); return VF_OK; }
// (n identity blocks scaled by 1 + the slot, so that a caller's copy shows which keyframe it asked for)
int vf_engine_read_marginals(vf_engine*, int w, int k0, int n, double* cov, double* cross) {
    logf("read_marginals w=%d k0=%d n=%d wants cov=%d cross=%d\n", w, k0, n, cov != nullptr, cross != nullptr);
    for (int i = 0; i < n; i++) {
        if (cov) { memset(cov + 225 * i, 0, 225 * sizeof(double)); for (int d = 0; d < 15; d++) cov[225 * i + 16 * d] = 1.0 + k0 + i; }
        if (cross) memset(cross + 225 * i, 0, 225 * sizeof(double));
    }
    return VF_OK;
}
}
