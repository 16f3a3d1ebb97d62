// vf_solve_plan.hpp -- which form the band solve (K4) of an engine takes, and what K3 and the marginals' factorisation do
// around it: one policy, decided here and nowhere else.  Host code without HIP (tests/native/solve_plan.cpp checks it on the CPU).
#pragma once

namespace vf {

// What the choice depends on: the batch and the engine's tuning (the View fields of the same names; vf_engine_tuning) and three
// facts about the engine
struct SolveInputs {
    int B, P, sh_G;                               // windows, chunks per window (>= 2: partitioned), ranks of a time-sharded window
    int tw_max, split_min, asm_min, asm_waves;
    bool hybrid;      // hybrid K4 (View::gate): the termination rule is on in a sweep engine that holds the partitioned form's buffers
    bool act_list;    // ... and the compacted list of the active windows (vf_engine_tuning.hybrid_active_list)
    bool vetoed;      // the solve reads H and g from K3: far factors alive, a refined solve, or GTSAM's accept rule (min_fidelity > 0)
    int simds = 0;    // SIMDs of the device, 4 per compute unit (0 = not known: no batch is "at most one window per SIMD")
    int bwd_form = 0; // vf_engine_tuning.solve_backsub_form: 0 = by batch, 1 = the two-per-SIMD form, 2 = the one-per-SIMD form
};
template <class View>
SolveInputs solve_inputs(const View& v, bool hybrid, bool act_list, bool vetoed) {
    return {v.B, v.P, v.sh_G, v.tw_max, v.split_min, v.asm_min, v.asm_waves, hybrid, act_list, vetoed, v.simds, v.bwd_form};
}

// whole-window sweeps
enum class Sweep {
    none,
    two_sided,   // k_band_solve_tw: two waves per window from both ends
    fused,       // k_band_solve: one wave per window
    split,       // k_band_forward + k_band_backward
    asm1,        // k_band_forward_asm + k_band_backward: the forward sweep assembles H itself
    asm2,        // k_band_forward_asm2 (launch_asm2) + k_band_backward: the same as an eliminator wave and an assembler wave
};
enum class K3 {
    all,           // k_assemble over every window
    partitioned,   // ... for the hybrid's partitioned half only (launch_assemble_for_partitioned)
    none,          // the sweep assembles: no K3
};
struct SolvePlan {
    int form;            // vf_engine_solve_form: 0 one wave, 1 split, 2 assembling, 3 two-sided, 4 partitioned, 5 hybrid
    Sweep sweep;         // the sweep over whole windows
    bool partitioned;    // the partitioned solve runs: alone, or as the hybrid's other half
    K3 k3;
    Sweep factor;        // vf_engine_marginals' factorisation, the forward half of a sweep: split (k_band_forward), asm1 or asm2
    bool bwd_one_wave = false;   // split, asm1, asm2: the back substitution is k_band_backward_1w, not k_band_backward
    bool hybrid() const { return partitioned && sweep != Sweep::none; }
};

// The back substitution behind a split or assembling forward sweep.  k_band_backward is built for two waves per SIMD (the partner
// wave covers a wave's LDS round trips; 256 registers); with at most one window per SIMD there is no partner, and
// k_band_backward_1w -- the recursion software-pipelined, four panels in flight, more registers -- takes the batch (the
// headline's 1 024 windows on 1 024 SIMDs: solve stage 3.46 -> 3.38 ms, NOTEBOOK.md 7.17).  Same bits either way.
inline bool backsub_one_wave(const SolveInputs& in, Sweep sweep) {
    if (sweep != Sweep::split && sweep != Sweep::asm1 && sweep != Sweep::asm2) return false;
    if (in.bwd_form == 1 || in.bwd_form == 2) return in.bwd_form == 2;
    return in.simds > 0 && in.B <= in.simds;
}

inline SolvePlan solve_plan_sweeps(const SolveInputs& in);
inline SolvePlan solve_plan(const SolveInputs& in) {
    SolvePlan p = solve_plan_sweeps(in);
    p.bwd_one_wave = backsub_one_wave(in, p.sweep);
    return p;
}
inline SolvePlan solve_plan_sweeps(const SolveInputs& in) {
    // the sweep assembles from this many windows on: one wave per window (the two-sided sweep takes the batches up to tw_max),
    // whole windows of an unsharded engine, and nothing in the solve that needs H
    const bool assembles = in.asm_min > 0 && in.B >= in.asm_min && in.P < 2 && in.B > in.tw_max && in.sh_G <= 1 && !in.vetoed;
    const Sweep asm_sweep = in.asm_waves == 2 ? Sweep::asm2 : Sweep::asm1;
    const Sweep one_wave = in.split_min > 0 && in.B >= in.split_min ? Sweep::split : Sweep::fused;
    if (in.P >= 2) return {4, Sweep::none, true, K3::all, Sweep::split};
    if (in.hybrid) {
        // The sweep half is never the two-sided one (k_band_solve_tw has no gate).  It takes two waves per window only with the
        // active list (round 5: with the compacted list, the eliminator's priority and -- what had made it 5 % slower than one
        // wave in round 4 and 21 % slower than itself in the headline's launch -- the placement kernel in front of it, launch_asm2)
        if (assembles) return {5, in.asm_waves == 2 && in.act_list ? Sweep::asm2 : Sweep::asm1, true, K3::partitioned, Sweep::split};
        return {5, one_wave, true, K3::all, Sweep::split};
    }
    if (in.B <= in.tw_max) return {3, Sweep::two_sided, false, K3::all, Sweep::split};
    if (assembles) return {2, asm_sweep, false, K3::none, asm_sweep};
    return {one_wave == Sweep::split ? 1 : 0, one_wave, false, K3::all, Sweep::split};
}

}  // namespace vf
