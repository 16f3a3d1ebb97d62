// vf_engine_memory.hpp -- what the device still holds from the last solve, and what voids it: one account, kept here and
// nowhere else.  Host code without HIP (tests/native/engine_memory.cpp checks it on the CPU).
//
// Five things outlive a solve on the device and let the next call do less: the linearisation of the current states (warm
// start: the next solve linearises only a tail), the panels and checkpoints of the incremental update, a marginal prior
// computed ahead of time, the result block an adaptive solve has already read, and what the covariance calls left (the blocks,
// the pose records, the scores: each only with the one before it).  A sixth outlives the arrays' next solve too: the last IMU-rate
// propagation (vf_engine_propagate_tail), which only a grown engine loses.  A seventh is a fact about the residuals rather than a
// saving: whether the current buffer's whitened residuals are those of the current states, so that vf_engine_factor_errors may read
// them as they lie (residuals_vouched), with the per-factor errors that call left (errors_valid).  An eighth is the innovation gate's result
// (vf_engine_gate_tail: gate_valid), which a compacted or grown engine loses; a ninth the loop-closure gate's (vf_engine_gate_closures:
// closure_gate_count), lost the same way.  Every entry point of the engine
// says what it did through one of the EVENTS below -- they are the only writers -- and asks through the QUERIES.
#pragma once

#include <algorithm>
#include <climits>

#include "../../include/vilfusion.h"

namespace vf {

// keyframes at a window's end that k_linearize_tail linearises again (one thread per keyframe, a handful of them): the
// longest tail a warm solve takes; a longer one is a cold start
constexpr int LINEARIZE_TAIL_MAX = 8;

class SolveMemory {
  public:
    // the facts about the engine the rules need: `slid` is one count for the whole engine, so appends are followed on
    // one-window engines only; time-sharded engines and vf_engine_opts.cold_start never start warm
    bool one_window = true, sharded = false, no_warm = false;
    // ... and two the residuals' fact needs: non-monotone LM restores states without their residuals (k_decide outcome 3,
    // k_close_excursion), and an incremental update linearises a suffix only -- such engines are never vouched for
    bool excursions = false, incremental = false;

    // ---- events.  lo / hi: window 0's range as it is when the event fires (the engine's own mirror, passed in, not kept here)
    // something the bookkeeping cannot follow was written: the next solve / update / marginalisation starts from nothing
    void rewritten() { forget(), res_current_ = false; }
    // records were written from slot k of window w onwards (an IMU record takes the fixed words of its own slot of the J stream with
    // it, both buffers, on the stream the record is written on: K0, k_fixed_jwords -- no other slot's words, so what holds for the
    // record holds for them).  At or beyond the end it is an append; up to LINEARIZE_TAIL_MAX slots
    // inside it (late odometry for a keyframe an earlier solve covered) the warm tail grows; the incremental update follows
    // a write anywhere behind the window's first keyframe.  Everything else is rewritten().
    void written_from(int w, int k, int lo, int hi) {
        // (a record at or beyond the end of the engine's one window is read by no residual the last solve left: an asynchronous
        // handle preintegrates the next keyframe's record while the last solve's errors are still wanted)
        if (!(one_window && w == 0 && k >= hi)) res_current_ = false;
        // (within a factor's reach of the first keyframe: it may be a factor the marginalisation of that keyframe reads)
        if (w == 0 && k <= lo + VF_MAX_BANDWIDTH) ahead_valid_ = false;
        if (!behind_first(w, k, lo) || !(warm_ || inc_valid_)) return forget();
        if (inc_valid_) inc_first_dirty_ = std::min(inc_first_dirty_, k);
        if (!warm_) return;
        redo_ = std::max(redo_, hi - k);          // (<= 0: beyond the current end)
        if (redo_ > LINEARIZE_TAIL_MAX) warm_ = false, ahead_valid_ = ahead_valid_ && inc_valid_;   // (inherited: an incremental engine keeps its stash here)
    }
    // the range of a window became [lo, hi); it was [old_lo, old_hi).  Growing the end of the one window of an engine is an
    // append of hi - old_hi keyframes (its start is moved by slid_by_one / vf_engine_drop_oldest only).
    void range_set(int lo, int hi, int old_lo, int old_hi) {
        res_current_ = false;
        if (!(one_window && lo == old_lo && hi >= old_hi && old_hi > old_lo)) return forget();
        if (warm_) slid_ += hi - old_hi;
        else ahead_valid_ = false;
        if (inc_valid_ && hi > old_hi) inc_first_dirty_ = std::min(inc_first_dirty_, old_hi);
    }
    // every window slid by one keyframe (vf_engine_slide): a change both the warm start and the incremental update follow
    void slid_by_one() { slid_ += warm_, inc_slid_ += inc_valid_, res_current_ = false; }
    // a solve ended: every record, H row and g entry is that of the current states.  Engines holding far factors start every
    // solve cold.  replayed: the solve was a hipGraph replay, which runs no host code of the stages -- the panels of the
    // incremental update and the stash survive it ("ahead_valid is voided only through cold()": the fix is
    // to drop the condition below).
    void solve_ended(bool far_alive, bool replayed) {
        if (!replayed) forget();
        warm_ = !no_warm && !far_alive;
        slid_ = redo_ = 0;
        residuals_current();
    }
    // an incremental update ended: its panels and checkpoints are those of the problem as it stands, or (failed) of nothing
    void inc_update_ended(bool ok) { rewritten(), inc_slid_ = 0, inc_first_dirty_ = INT_MAX, inc_valid_ = ok; }
    // every factor of every window has just been linearised at the current states into the current buffer, and nothing has moved
    // since: a solve that ended, a finished vf_engine_isam_step or vf_engine_linearize(e, 0), vf_engine_marginals_ex, the
    // relinearising path of vf_engine_factor_errors
    void residuals_current() { res_current_ = !excursions && !incremental; }
    // states from slot k of window w onwards were predicted from the estimate: a rewrite for the warm start and the stash,
    // an append for the incremental update if it lies behind the first keyframe of a one-window engine
    void predicted_from_estimate(int w, int k, int lo) {
        if (inc_valid_ && behind_first(w, k, lo)) inc_first_dirty_ = std::min(inc_first_dirty_, k);
        else inc_valid_ = false;
        warm_ = ahead_valid_ = res_current_ = false;
    }
    // the window was compacted: the covariance blocks stay in the slots they were computed for
    void compacted() { rewritten(), covariances_started(), err_valid_ = gate_valid_ = false, closure_n_ = 0; }
    // the engine was grown: new arrays, nothing linearised in them yet, no covariances
    void grown() { rewritten(), covariances_started(), slid_ = redo_ = 0, prop_valid_ = prop_cov_ = err_valid_ = gate_valid_ = false, closure_n_ = 0; }
    // the marginal prior of the keyframe at `lo` was computed ahead of time / ... was put in place
    void stashed(int lo) { ahead_valid_ = true, ahead_lo_ = lo; }
    void stash_committed() { ahead_valid_ = false; }
    // the result block of window 0, slot s is in the pinned buffer; sticky words an early read consumed wait for the final one
    void result_cached(int slot) { res_cached_ = true, res_slot_ = slot; }
    void sticky_consumed(int s0, int s1) { res_carry_[0] |= s0, res_carry_[1] |= s1; }
    void sticky_handed_on(int* s0, int* s1) {
        *s0 |= res_carry_[0], *s1 |= res_carry_[1];
        res_carry_[0] = res_carry_[1] = 0;
    }
    // an entry point ran: the cached result is void, unless the entry point leaves the result block alone
    void entry_ran(bool leaves_result) { res_cached_ = res_cached_ && leaves_result; }
    // vf_engine_marginals_ex is about to free or overwrite what the last one left: void from here on, whether or not it gets through
    void covariances_started() { sig_valid_ = pose_valid_ = sig_tail_ = false, score_rows_ = 0; }
    // ... it got through, with the pose records (VF_MARGINALS_POSE) or, as the plain vf_engine_marginals, without; scores are of the
    // records of one call: none yet
    void covariances_computed(bool pose = false) { sig_valid_ = true, pose_valid_ = pose, sig_tail_ = false, score_rows_ = 0, residuals_current(); }
    // ... it got through with VF_MARGINALS_TAIL: the blocks of every window's last two keyframes only, no pose records
    void covariances_computed_tail() { covariances_computed(false), sig_tail_ = true; }
    // vf_engine_marginal_scores left `rows` rows of scores (0: it is about to overwrite them)
    void scores_computed(int rows) { score_rows_ = rows; }
    // vf_engine_propagate_tail left a propagation in its own buffer, with or without the covariance.  It is of the arrays it was
    // enqueued on: nothing but grown() voids it
    void propagated(bool cov) { prop_valid_ = true, prop_cov_ = cov; }
    // vf_engine_factor_errors is about to overwrite what the last one left / left the errors of every window in its own buffer.
    // They are of the call that wrote them: later solves leave them, a compacted or grown engine loses them
    void errors_started() { err_valid_ = false; }
    void errors_computed() { err_valid_ = true; }
    // vf_engine_gate_tail left a result for every window in its own buffer.  It is of the call that wrote it: later solves leave
    // it, a compacted or grown engine loses it
    void gated() { gate_valid_ = true; }
    // vf_engine_gate_closures left n records (and joint covariances) in its own buffer.  They are of the call that wrote them, as
    // the tail gate's: later solves leave them, a compacted or grown engine loses them
    void closure_gated(int n) { closure_n_ = n; }

    // ---- queries
    // keyframes at the window's end the next solve linearises again, 0: a cold solve (everything).  The launch sequence of
    // vf_engine_iterate and the key of its captured graph both take it from here.
    int tail() const { return warm_ && !sharded && slid_ + redo_ >= 1 && slid_ + redo_ <= LINEARIZE_TAIL_MAX ? slid_ + redo_ : 0; }
    bool is_warm() const { return warm_; }
    // the next incremental update eliminates the whole window / how many keyframes at the end of [lo, hi) are new to it
    bool inc_whole_window() const { return !inc_valid_; }
    int inc_appended(int hi) const { return one_window && inc_first_dirty_ != INT_MAX ? std::max(inc_slid_, hi - inc_first_dirty_) : inc_slid_; }
    bool inc_slid() const { return inc_slid_ > 0; }
    bool stash_fits(int lo) const { return ahead_valid_ && ahead_lo_ == lo; }
    bool result_cached_for(int window, int slot, bool estimate) const { return res_cached_ && window == 0 && slot == res_slot_ && !estimate; }
    bool covariances_valid() const { return sig_valid_; }
    bool pose_records_valid() const { return sig_valid_ && pose_valid_; }
    int score_rows() const { return pose_records_valid() ? score_rows_ : 0; }
    bool propagation_valid() const { return prop_valid_; }
    bool propagated_covariance_valid() const { return prop_valid_ && prop_cov_; }
    // the current buffer's residuals are those of the current states (never on engines with excursions or incremental updates)
    bool residuals_vouched() const { return res_current_ && !excursions && !incremental; }
    bool errors_valid() const { return err_valid_; }
    // the covariances are valid, but of every window's tail only (its last two keyframes)
    bool covariances_tail_only() const { return sig_valid_ && sig_tail_; }
    bool gate_valid() const { return gate_valid_; }
    // records the last vf_engine_gate_closures left to be read (0: none)
    int closure_gate_count() const { return closure_n_; }

  private:
    // what rewritten() does to the savings, for the events that are rewrites inside but say themselves what becomes of the residuals
    void forget() { warm_ = inc_valid_ = ahead_valid_ = false; }
    bool behind_first(int w, int k, int lo) const { return one_window && w == 0 && k > lo; }
    bool warm_ = false;
    int slid_ = 0, redo_ = 0;     // keyframes appended since the last solve / slots in front of the old end whose factors changed
    bool inc_valid_ = false;      // the panels are those of the problem after the last update, and all that changed since is an append:
    int inc_slid_ = 0, inc_first_dirty_ = INT_MAX;      // ... that many slides, or writes at or beyond this slot
    bool ahead_valid_ = false;
    int ahead_lo_ = -1;
    bool res_cached_ = false;
    int res_slot_ = -1, res_carry_[2] = {0, 0};
    bool sig_valid_ = false, pose_valid_ = false;
    int score_rows_ = 0;
    bool prop_valid_ = false, prop_cov_ = false;
    bool res_current_ = false, err_valid_ = false;
    bool sig_tail_ = false, gate_valid_ = false;
    int closure_n_ = 0;
};

}  // namespace vf
