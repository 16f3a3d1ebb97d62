// Which back substitution kernel follows a split or assembling forward sweep (vf_solve_plan.hpp, backsub_one_wave): the form built
// for one wave per SIMD up to one window per SIMD of the device, the two-per-SIMD form above, either one when
// vf_engine_tuning.solve_backsub_form forces it -- and nothing else about a plan moves.  The table of solve_plan.cpp is run first, as
// it stands (its inputs leave the two new ones at their defaults): tests/test_solve_plan_backsub_host.py.
#include <initializer_list>

#define main solve_plan_table_main
#include "solve_plan.cpp"
#undef main

namespace {

SolveInputs on_device(SolveInputs in, int simds, int bwd_form = 0) {
    in.simds = simds;
    in.bwd_form = bwd_form;
    return in;
}
bool same_but_backsub(const SolvePlan& a, const SolvePlan& b) {
    return a.form == b.form && a.sweep == b.sweep && a.partitioned == b.partitioned && a.k3 == b.k3 && a.factor == b.factor && a.hybrid() == b.hybrid();
}

}  // namespace

int main() {
    if (int rc = solve_plan_table_main()) return rc;
    int bad = 0;
    auto expect = [&](const char* what, const SolveInputs& in, bool one_wave) {
        const SolvePlan p = vf::solve_plan(in);
        SolveInputs plain = in;
        plain.simds = 0;
        plain.bwd_form = 0;
        const SolvePlan q = vf::solve_plan(plain);
        if (p.bwd_one_wave != one_wave || q.bwd_one_wave || !same_but_backsub(p, q)) {
            std::printf("%s: bwd_one_wave %d, expected %d; with the defaults %d, expected 0; rest of the plan %s\n", what, (int)p.bwd_one_wave,
                        (int)one_wave, (int)q.bwd_one_wave, same_but_backsub(p, q) ? "unchanged" : "CHANGED");
            bad++;
        }
    };
    const int S = 1024;      // an MI355X: 256 compute units
    // the three sweeps that end in the back substitution kernel, around one window per SIMD
    const SolveInputs asm2 = with(at(1), 1, 0, 0, 1, 2), asm1 = with(at(1), 1, 0, 0, 1, 1), split = with(at(1), 1, 0, 1, 0, 2);
    for (const SolveInputs& base : {asm2, asm1, split}) {
        for (int B : {1, S - 1, S, S + 1, 4 * S}) {
            SolveInputs in = base;
            in.B = B;
            expect("by batch", on_device(in, S), B <= S);
            expect("device not known", on_device(in, 0), false);
            expect("forced two-per-SIMD", on_device(in, S, 1), false);
            expect("forced one-per-SIMD", on_device(in, S, 2), true);
            expect("forced one-per-SIMD, device not known", on_device(in, 0, 2), true);
            expect("a field value the library does not know", on_device(in, S, 7), B <= S);
        }
    }
    // the library's defaults at the headline batch and beside it
    expect("defaults, 1023 windows", on_device(at(S - 1), S), true);
    expect("defaults, 1024 windows", on_device(at(S), S), true);
    expect("defaults, 1025 windows", on_device(at(S + 1), S), false);
    expect("defaults, 1024 windows, 304 compute units", on_device(at(S), 1216), true);
    expect("defaults, 2048 windows, asm_min 0 (split)", on_device(with(at(2048), 1, 256, 2048, 0, 2), S), false);
    // the sweep half of a hybrid solve ends in the same kernel
    expect("hybrid, 1024 windows", on_device(at(S, 0, true, true), S), true);
    expect("hybrid, 2048 windows, asm_min 0", on_device(with(at(2048, 0, true), 1, 256, 2048, 0, 2), S), false);
    expect("hybrid, 2048 windows, asm_min 0, forced", on_device(with(at(2048, 0, true), 1, 256, 2048, 0, 2), S, 2), true);
    // plans without that kernel never ask for a form of it, forced or not
    for (int form : {0, 1, 2}) {
        expect("partitioned", on_device(at(64, 96), S, form), false);
        expect("two-sided", on_device(at(200), S, form), false);
        expect("fused", on_device(at(300), S, form), false);
        expect("fused, vetoed", on_device(at(1024, 0, false, true, true), S, form), false);
        expect("hybrid, fused half", on_device(at(300, 0, true), S, form), false);
    }
    if (bad) return 1;
    std::printf("solve_plan backsub ok\n");
    return 0;
}
