// How the View of one launch may differ from the engine's (vil_sensor_fusion_amd/csrc/vf_launch_view.hpp), as a table: every variant
// and every composition the engine launches is applied to a View of patterned bytes, and the result is compared byte by byte --
// the fields the variant owns hold the listed values, every other byte of the 712 is the base's.
//
// The expectations are NOT derived from the header: each is what the engine's host code assigned by hand before the header
// existed (the commit before "one account of how a launch's View differs"): engine/engine_errors.inc:27-30, engine_marginals.inc:55-64,
// engine_window.inc:26 and :51, engine_read.inc:157, engine_compat.inc:40-43, engine_solve.inc:49-57, :119-122, :203, :232,
// engine_shard.inc:87 and :97, kernels/launch.inc:63, :75-79, :131-135, vf_engine::partitioned_view().
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "vf_launch_view.hpp"

namespace {
using vf::View;
static_assert(sizeof(View) == 712, "the kernel argument block");
int failures = 0;

// one field a variant owns: where it is, and the bytes it must hold
struct Own {
    size_t off, size;
    unsigned char val[8];
};
template <class T>
Own own(size_t off, T value) {
    static_assert(sizeof(T) <= 8, "a word or a pointer");
    Own o{off, sizeof(T), {0}};
    memcpy(o.val, &value, sizeof(T));
    return o;
}
#define OWN(field, value) own<decltype(View::field)>(offsetof(View, field), (value))

struct Variant {
    std::string name;
    std::function<View(View)> apply;
    std::vector<Own> owns;
    bool constant_word;      // sets a word whose neutral value is a constant: launch_words_neutral() must see it
};

View base_view() {
    // a non-trivial pattern in every byte, padding included; then the launch words at their constant neutral values
    unsigned char raw[sizeof(View)];
    for (size_t i = 0; i < sizeof(View); i++) raw[i] = (unsigned char)(0x35 + 7 * i + (i >> 3));
    View v;
    memcpy(&v, raw, sizeof(View));
    v.gate = 0;
    v.act = nullptr;
    v.inc_on = 0;
    v.inc_prior = 0;
    v.relin_only = 0;
    v.w_first = 0;
    v.stop_on = 1;          // (an engine under the termination rule: the variants that switch it off must show)
    return v;
}

void check(const std::string& what, const View& got, const View& base, const std::vector<Own>& owns) {
    unsigned char g[sizeof(View)], want[sizeof(View)];
    memcpy(g, &got, sizeof(View));
    memcpy(want, &base, sizeof(View));
    for (const Own& o : owns) memcpy(want + o.off, o.val, o.size);
    for (size_t i = 0; i < sizeof(View); i++)
        if (g[i] != want[i]) {
            failures++;
            printf("FAIL %s: byte %zu is 0x%02x, want 0x%02x\n", what.c_str(), i, g[i], want[i]);
            return;
        }
}

bool disjoint(const std::vector<Own>& a, const std::vector<Own>& b) {
    for (const Own& x : a)
        for (const Own& y : b)
            if (x.off < y.off + y.size && y.off < x.off + x.size) return false;
    return true;
}
std::vector<Own> both(std::vector<Own> a, const std::vector<Own>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
}  // namespace

int main() {
    const View base = base_view();
    // the arrays a launch is pointed at: addresses only, never read
    static double rhs[4], inc[4], zeros[4], Vp[4], sep[3 * vf::SEPM], sepL[4];
    static int stop[4], failed[4], ones[4], list[4];

    const std::vector<Variant> table = {
        {"1 every_window", [](View v) { return vf::every_window(v); }, {OWN(stop_on, 0)}, false},
        {"2 on_buffers", [](View v) { return vf::on_buffers(v, rhs, inc); }, {OWN(gvec, rhs), OWN(delta, inc)}, false},
        {"2 on_buffers (increment only, skip)", [](View v) { return vf::on_buffers(v, nullptr, inc, stop); },
         {OWN(delta, inc), OWN(stop_on, 1), OWN(done, stop)}, false},
        {"2 on_buffers (skip)", [](View v) { return vf::on_buffers(v, rhs, inc, stop); },
         {OWN(gvec, rhs), OWN(delta, inc), OWN(stop_on, 1), OWN(done, stop)}, false},
        {"3 restored_only", [](View v) { return vf::restored_only(v); }, {OWN(relin_only, 1)}, true},
        {"4 from_active_list", [](View v) { return vf::from_active_list(v, list); }, {OWN(act, list)}, true},
        {"5 incremental", [](View v) { return vf::incremental(v, false); }, {OWN(inc_on, 1), OWN(inc_prior, 0), OWN(stop_on, 0)}, true},
        {"5 incremental (priors)", [](View v) { return vf::incremental(v, true); }, {OWN(inc_on, 1), OWN(inc_prior, 1), OWN(stop_on, 0)}, true},
        {"6 undamped_whole", [](View v) { return vf::undamped_whole(v, zeros, failed, ones); },
         {OWN(lambda, zeros), OWN(fail, failed), OWN(fresh, ones), OWN(P, 0), OWN(stop_on, 0)}, false},
        {"7 hybrid_half (sweep)", [](View v) { return vf::hybrid_half(v, 1); }, {OWN(gate, 1)}, true},
        {"7 hybrid_half (partitioned)", [](View v) { return vf::hybrid_half(v, 2); }, {OWN(gate, 2)}, true},
        {"8 one_window_k3", [](View v) { return vf::one_window_k3(v, 5); }, {OWN(gate, 2), OWN(gate_T, 1 << 30), OWN(w_first, 5), OWN(stop_on, 0)}, true},
        {"9 partitioned_form", [](View v) { return vf::partitioned_form(v, 8, Vp, sep, sepL); },
         {OWN(P, 8), OWN(P_fit, 1), OWN(Vp, Vp), OWN(sepR, sep), OWN(sepS, sep + vf::SEPM), OWN(sepC, sep + 2 * vf::SEPM), OWN(sepL, sepL)}, false},
    };

    if (!vf::launch_words_neutral(base)) { failures++; printf("FAIL launch_words_neutral(base) is false\n"); }
    for (const Variant& a : table) {
        const View got = a.apply(base);
        check(a.name, got, base, a.owns);
        if (vf::launch_words_neutral(got) != !a.constant_word) {
            failures++;
            printf("FAIL %s: launch_words_neutral is %d\n", a.name.c_str(), (int)vf::launch_words_neutral(got));
        }
    }
    // compositions: wherever two variants own disjoint words, either order gives the same bytes -- the words of both, the base's elsewhere
    // (this is what a variant that resets a word it does not own fails)
    int pairs = 0;
    for (const Variant& a : table)
        for (const Variant& b : table) {
            if (&a == &b || !disjoint(a.owns, b.owns)) continue;
            pairs++;
            check(a.name + " o " + b.name, a.apply(b.apply(base)), base, both(a.owns, b.owns));
        }
    // ... and the ones the engine launches.  solve(): the sweep half of a hybrid on another right-hand side (2 o 4, then 7 in
    // launch_band_solve), its partitioned half (2 o 9, then 7)
    const std::vector<Own> o2 = table[3].owns, o4 = table[5].owns, o9 = table[12].owns;
    check("solve: sweep half", vf::hybrid_half(vf::from_active_list(vf::on_buffers(base, rhs, inc, stop), list), 1), base,
          both(both(o2, o4), {OWN(gate, 1)}));
    check("solve: partitioned half", vf::hybrid_half(vf::on_buffers(vf::partitioned_form(base, 8, Vp, sep, sepL), rhs, inc, stop), 2), base,
          both(both(o2, o9), {OWN(gate, 2)}));
    check("solve: 2 o 4 o 9", vf::on_buffers(vf::from_active_list(vf::partitioned_form(base, 8, Vp, sep, sepL), list), rhs, inc, stop), base,
          both(both(o2, o4), o9));
    // vf_engine_time_stage: K4 as the View alone gives it, on every window (1, then launch_band_solve without a hybrid: no gate)
    check("time_stage", vf::every_window(base), base, {OWN(stop_on, 0)});
    // vf_engine_marginals_ex: every later launch of the call takes the one copy (6)
    check("marginals", vf::undamped_whole(base, zeros, failed, ones), base, table[8].owns);

    if (failures) {
        printf("launch_view: %d failure(s)\n", failures);
        return 1;
    }
    printf("launch_view ok (%zu variants, %d ordered pairs)\n", table.size(), pairs);
    return 0;
}
