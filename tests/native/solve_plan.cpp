// The K4 form, K3 and the marginals' factor kernel as vf_solve_plan.hpp decides them, against a table (tests/test_solve_plan_host.py).
// No device: the policy is host code.  Library defaults: sweep_two_sided_max 256, solve_split_min 2048, solve_assemble_min 768,
// solve_assemble_waves 2, hybrid_active_list on; chunks = 0 gives the partitioned form up to 128 windows.
#include <cstdio>

#include "vf_solve_plan.hpp"

using vf::K3;
using vf::SolveInputs;
using vf::SolvePlan;
using vf::Sweep;

namespace {

struct Row {
    const char* what;
    SolveInputs in;
    int form;
    Sweep sweep;
    bool partitioned;
    K3 k3;
    Sweep factor;
};

// defaults, changed by the arguments that follow B
SolveInputs at(int B, int P = 0, bool hybrid = false, bool act_list = true, bool vetoed = false) {
    return {B, P, 1, 256, 2048, 768, 2, hybrid, act_list, vetoed};
}
SolveInputs with(SolveInputs in, int sh_G, int tw_max, int split_min, int asm_min, int asm_waves) {
    in.sh_G = sh_G;
    in.tw_max = tw_max;
    in.split_min = split_min;
    in.asm_min = asm_min;
    in.asm_waves = asm_waves;
    return in;
}

const char* name(Sweep s) {
    switch (s) {
        case Sweep::none: return "none";
        case Sweep::two_sided: return "two_sided";
        case Sweep::fused: return "fused";
        case Sweep::split: return "split";
        case Sweep::asm1: return "asm1";
        case Sweep::asm2: return "asm2";
    }
    return "?";
}
const char* name(K3 k) { return k == K3::all ? "all" : k == K3::partitioned ? "partitioned" : "none"; }

}  // namespace

int main() {
    const Row rows[] = {
        // partitioned whenever P >= 2, at any batch
        {"partitioned, 2 windows", at(2, 96), 4, Sweep::none, true, K3::all, Sweep::split},
        {"partitioned, 128 windows", at(128, 96), 4, Sweep::none, true, K3::all, Sweep::split},
        {"partitioned, 1024 windows, chunks 4", at(1024, 4), 4, Sweep::none, true, K3::all, Sweep::split},
        {"partitioned, vetoed", at(1024, 4, false, true, true), 4, Sweep::none, true, K3::all, Sweep::split},
        // two-sided up to tw_max, even where the sweep could assemble
        {"two-sided, 129 windows", at(129), 3, Sweep::two_sided, false, K3::all, Sweep::split},
        {"two-sided, 256 windows", at(256), 3, Sweep::two_sided, false, K3::all, Sweep::split},
        {"two-sided, asm_min 1", with(at(200), 1, 256, 2048, 1, 2), 3, Sweep::two_sided, false, K3::all, Sweep::split},
        // one wave per window
        {"fused, 300 windows", at(300), 0, Sweep::fused, false, K3::all, Sweep::split},
        {"fused, 767 windows", at(767), 0, Sweep::fused, false, K3::all, Sweep::split},
        {"assembling-2, 768 windows", at(768), 2, Sweep::asm2, false, K3::none, Sweep::asm2},
        {"assembling-2, 1024 windows", at(1024), 2, Sweep::asm2, false, K3::none, Sweep::asm2},
        {"assembling-2, 2048 windows", at(2048), 2, Sweep::asm2, false, K3::none, Sweep::asm2},
        {"assembling-1, 1024 windows", with(at(1024), 1, 256, 2048, 768, 1), 2, Sweep::asm1, false, K3::none, Sweep::asm1},
        {"assembling-2, one window, tw_max 0", with(at(1), 1, 0, 2048, 1, 2), 2, Sweep::asm2, false, K3::none, Sweep::asm2},
        {"split, 2048 windows, asm_min 0", with(at(2048), 1, 256, 2048, 0, 2), 1, Sweep::split, false, K3::all, Sweep::split},
        {"fused, 2047 windows, asm_min 0", with(at(2047), 1, 256, 2048, 0, 2), 0, Sweep::fused, false, K3::all, Sweep::split},
        {"fused, 4096 windows, split_min 0, asm_min 0", with(at(4096), 1, 256, 0, 0, 2), 0, Sweep::fused, false, K3::all, Sweep::split},
        // a veto (far factors, refined solve, GTSAM's accept rule) keeps K3 and the sweep that reads H
        {"vetoed, 1024 windows", at(1024, 0, false, true, true), 0, Sweep::fused, false, K3::all, Sweep::split},
        {"vetoed, 2048 windows", at(2048, 0, false, true, true), 1, Sweep::split, false, K3::all, Sweep::split},
        {"vetoed, 1024 windows, asm_waves 1", with(at(1024, 0, false, true, true), 1, 256, 2048, 768, 1), 0, Sweep::fused, false, K3::all, Sweep::split},
        // hybrid: the sweep half is never two-sided; it assembles only with K3 for the partitioned half, two waves only with the list
        {"hybrid, 200 windows", at(200, 0, true), 5, Sweep::fused, true, K3::all, Sweep::split},
        {"hybrid, 200 windows, asm_min 1", with(at(200, 0, true), 1, 256, 2048, 1, 2), 5, Sweep::fused, true, K3::all, Sweep::split},
        {"hybrid, 300 windows", at(300, 0, true), 5, Sweep::fused, true, K3::all, Sweep::split},
        {"hybrid, 1024 windows, active list", at(1024, 0, true, true), 5, Sweep::asm2, true, K3::partitioned, Sweep::split},
        {"hybrid, 1024 windows, no active list", at(1024, 0, true, false), 5, Sweep::asm1, true, K3::partitioned, Sweep::split},
        {"hybrid, 1024 windows, asm_waves 1", with(at(1024, 0, true, true), 1, 256, 2048, 768, 1), 5, Sweep::asm1, true, K3::partitioned, Sweep::split},
        {"hybrid, 1024 windows, vetoed", at(1024, 0, true, true, true), 5, Sweep::fused, true, K3::all, Sweep::split},
        {"hybrid, 2048 windows, vetoed", at(2048, 0, true, true, true), 5, Sweep::split, true, K3::all, Sweep::split},
        {"hybrid, 2048 windows, asm_min 0", with(at(2048, 0, true), 1, 256, 2048, 0, 2), 5, Sweep::split, true, K3::all, Sweep::split},
        // time-sharded engines never assemble
        {"sharded, 8 windows, chunks 8", with(at(8, 8), 2, 256, 2048, 768, 2), 4, Sweep::none, true, K3::all, Sweep::split},
        {"sharded, 1024 windows, no chunks", with(at(1024), 2, 256, 2048, 768, 2), 0, Sweep::fused, false, K3::all, Sweep::split},
        {"sharded, 2048 windows, no chunks", with(at(2048), 2, 256, 2048, 768, 2), 1, Sweep::split, false, K3::all, Sweep::split},
    };
    int bad = 0;
    for (const Row& r : rows) {
        const SolvePlan p = vf::solve_plan(r.in);
        if (p.form != r.form || p.sweep != r.sweep || p.partitioned != r.partitioned || p.k3 != r.k3 || p.factor != r.factor ||
            p.hybrid() != (r.form == 5)) {
            std::printf("%s: form %d sweep %s partitioned %d K3 %s factor %s; expected form %d sweep %s partitioned %d K3 %s factor %s\n",
                        r.what, p.form, name(p.sweep), (int)p.partitioned, name(p.k3), name(p.factor), r.form, name(r.sweep),
                        (int)r.partitioned, name(r.k3), name(r.factor));
            bad++;
        }
    }
    if (bad) return 1;
    std::printf("solve_plan ok (%d rows)\n", (int)(sizeof(rows) / sizeof(rows[0])));
    return 0;
}
