// vf_launch_view.hpp -- how the View of ONE launch may differ from the engine's: the list, decided here and nowhere else.
// Host code (tests/native/launch_view.cpp checks it on the CPU, byte by byte).
//
// vf::View is the engine's state -- arrays, LM constants, the far lists -- and a handful of words that are arguments of a launch:
//
//   words                              neutral: what vf_engine::v holds       read by
//   stop_on, done                      the termination rule's, the engine's   window_done(), K3's w_done, k_count_active, k_read_result
//   gate, gate_T                       0, the hybrid's threshold              gated_off(); K3 ignores `fresh` under gate == 2
//   act                                null                                   sweep_window(); k_count_active fills it
//   inc_on, inc_prior                  0, 0                                   early returns of K1 / K2 / K2b, K3's row range and `fresh`
//   relin_only                         0                                      early returns of K1 / K2 / K2b
//   w_first                            0                                      K3's window index
//   gvec, delta                        the engine's arrays                    K4 and what follows it
//   lambda, fail, fresh                the engine's arrays                    K4's damping and failure flags, K3's `fresh`
//   P, P_fit, Vp, sepR/S/C, sepL       the engine's own K4 form               the chunk kernels, own_range()
//
// The invariant: vf_engine::v holds the neutral value of every one of them at all times.  A launch that needs another value gets a
// COPY made by one of the functions below, each of which writes the words it owns and no other -- none resets what it does not own:
// the invariant makes that unnecessary, and they compose (vf_engine's solve() launches 2 o 4 o 9).  What the engine does assign in
// its own View is engine state, not launch words: creation and vf_engine_grow, vf_engine_set_convergence (stop_on and the
// tolerances), attach_far / ensure_far, ensure_excursion, ensure_loss (btw_loss / btw_loss_k, the robust losses' arrays: the launchers
// choose the K2 kernels by them), vf_engine_set_shard, sh_all_jac in linearize(), nm_W in decide().
#pragma once
#include "vf_kernels.hpp"

namespace vf {

// ... as far as a View alone can tell: the words whose neutral value is a constant (the others are neutral when they are the engine's)
inline bool launch_words_neutral(const View& v) {
    return v.gate == 0 && v.act == nullptr && v.inc_on == 0 && v.inc_prior == 0 && v.relin_only == 0 && v.w_first == 0;
}

// 1. every window, whether or not the termination rule has finished it
inline View every_window(View v) { v.stop_on = 0; return v; }
// 2. another right-hand side and / or increment buffer (null: the engine's); skip: windows flagged there take no part
inline View on_buffers(View v, double* gvec, double* delta, const int* skip = nullptr) {
    if (gvec) v.gvec = gvec;
    if (delta) v.delta = delta;
    if (skip) { v.stop_on = 1; v.done = const_cast<int*>(skip); }
    return v;
}
// 3. restored windows only (View::relin)
inline View restored_only(View v) { v.relin_only = 1; return v; }
// 4. one-wave sweeps take their windows from the compacted list of the active ones; k_count_active writes it
inline View from_active_list(View v, int* act) { v.act = act; return v; }
// 5. incremental update: K1 / K2 / K3 from inc_k[w] on, the priors too if asked
inline View incremental(View v, bool priors) { v.inc_on = 1; v.inc_prior = priors ? 1 : 0; return every_window(v); }
// 6. undamped whole-window factorisation of every window on the caller's arrays (lambda: zeros, fresh: ones)
inline View undamped_whole(View v, double* lambda, int* fail, int* fresh) {
    v.lambda = lambda; v.fail = fail; v.fresh = fresh; v.P = 0;
    return every_window(v);
}
// 7. the halves of a hybrid K4 (View::gate): 1 = the sweep, 2 = the partitioned form (K3 for it alone: launch_assemble_for_partitioned)
inline View hybrid_half(View v, int half) { v.gate = half; return v; }
// 8. K3 of one window on demand: gate 2 so that it ignores `fresh`, a threshold under which a gate-2 launch always runs
inline View one_window_k3(View v, int window) { v.gate = 2; v.gate_T = 1 << 30; v.w_first = window; return every_window(v); }
// 9. the partitioned form of a sweep engine (vf_engine::partitioned_view hands in the hybrid's buffers; sep: one buffer of SEPK slots)
inline View partitioned_form(View v, int P, double* Vp, double* sep, double* sepL) {
    v.P = P; v.P_fit = 1; v.Vp = Vp; v.sepR = sep; v.sepS = sep + SEPM; v.sepC = sep + 2 * SEPM; v.sepL = sepL;
    return v;
}

}  // namespace vf
