// What a solve leaves on the device and what voids it (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp), as a table of event
// sequences with the answer of every query after each event.
//
// The expectations are NOT derived from the header: each is what the engine's host code did before the header existed, where
// the same rules were spread over loose fields of struct vf_engine.  The comment on every case names the lines of that code
// (the commit "Split vf_solve into named steps over one snapshot of what it took") the expectation was read from:
//   cold()            vf_engine.hip:387-391            DeviceGuard (voids the cached result)  vf_engine.hip:393-400
//   touch()           engine/engine_staging.inc:11-31  vf_engine_set_range   engine/engine_staging.inc:48-62
//   vf_engine_read_result  engine/engine_staging.inc:84   tail of a warm solve  engine/engine_solve.inc:264-265 and :329
//   mark_solved()     engine/engine_solve.inc:313-317  res_cached set        engine/engine_solve.inc:308
//   isam_step_incremental  engine/engine_compat.inc:30-54   vf_engine_predict_from_estimate  engine/engine_compat.inc:94
//   marginalize / _ahead   engine/engine_window.inc:11-17, :187, :201-202    vf_engine_slide  engine/engine_window.inc:248-249
//   vf_engine_compact engine/engine_window.inc:281-285 vf_engine_grow        engine/engine_window.inc:472-473
//   vf_engine_marginals    engine/engine_marginals.inc:24-26, :62, :101
#include <cstdio>

#include "vf_engine_memory.hpp"

namespace {
int failures = 0;
// the window [lo, hi) of the engine's window 0, kept by the test as the engine keeps h_lo / h_hi
struct Rig {
    vf::SolveMemory m;
    int lo = 100, hi = 140;
    const char* name;
    explicit Rig(const char* n, bool one_window = true, bool sharded = false, bool no_warm = false) : name(n) {
        m.one_window = one_window;
        m.sharded = sharded;
        m.no_warm = no_warm;
    }
    // tail, warm, whole-window update, appended keyframes, stash fits lo, result cached for (0, hi - 1, state), covariances
    void expect(const char* step, int tail, bool warm, bool whole, int appended, bool stash, bool cached, bool cov) {
        const bool ok = m.tail() == tail && m.is_warm() == warm && m.inc_whole_window() == whole && m.inc_appended(hi) == appended &&
                        m.stash_fits(lo) == stash && m.result_cached_for(0, hi - 1, false) == cached && m.covariances_valid() == cov;
        if (ok) return;
        failures++;
        printf("FAIL %s / %s: tail %d (want %d) warm %d (%d) whole %d (%d) appended %d (%d) stash %d (%d) cached %d (%d) cov %d (%d)\n", name, step,
               m.tail(), tail, m.is_warm(), warm, m.inc_whole_window(), whole, m.inc_appended(hi), appended, m.stash_fits(lo), stash,
               m.result_cached_for(0, hi - 1, false), cached, m.covariances_valid(), cov);
    }
    // what the covariance calls left: the blocks, the pose records, rows of scores
    void expect_cov(const char* step, bool cov, bool pose, int rows) {
        if (m.covariances_valid() == cov && m.pose_records_valid() == pose && m.score_rows() == rows) return;
        failures++;
        printf("FAIL %s / %s: covariances %d (want %d) pose records %d (%d) score rows %d (%d)\n", name, step, m.covariances_valid(), cov,
               m.pose_records_valid(), pose, m.score_rows(), rows);
    }
    void write(int w, int k) { m.written_from(w, k, lo, hi); }
    void range(int nlo, int nhi) { m.range_set(nlo, nhi, lo, hi); lo = nlo; hi = nhi; }
    void slide() { m.slid_by_one(); lo++; hi++; }
    void solved(bool far = false, bool replayed = false) { m.solve_ended(far, replayed); }
    void updated(bool ok = true) { m.inc_update_ended(ok); }
};
enum Kind { WARM, INC, BOTH };
Rig make(const char* name, Kind k) {
    Rig r(name);
    if (k != WARM) r.updated();          // compat.inc:44-54: cold, counters reset, inc_valid = true
    if (k != INC) r.solved();            // with the stages' cold() inside the solve (solve.inc:5-7): inc_valid goes, see below
    if (k == BOTH) {
        // an engine that is both: the update ran last and the warm flag was then set by a replayed solve (solve.inc:354-356, no cold())
        r.updated();
        r.solved(false, true);
    }
    return r;
}
}  // namespace

int main() {
    {   // a fresh engine: nothing is remembered; a solve makes it warm (solve.inc:313-317), and voids the incremental panels
        // through the cold() of its stages (solve.inc:5-7)
        Rig r("fresh");
        r.expect("created", 0, false, true, 0, false, false, false);
        r.updated();
        r.expect("update", 0, false, false, 0, false, false, false);
        r.solved();
        r.expect("solve", 0, true, true, 0, false, false, false);
        r.updated(false);      // compat.inc:52-53: a failed update returns before inc_valid = true; :44 has gone cold
        r.expect("failed update", 0, false, true, 0, false, false, false);
    }
    {   // append at the end, warm engine: touch() :25-28 inside = 0, redo stays 0: still warm, tail counts slides (window.inc:248)
        Rig r = make("append warm", WARM);
        r.write(0, r.hi);
        r.expect("write at hi", 0, true, true, 0, false, false, false);       // tail 0: slid + redo = 0 (solve.inc:265: tail >= 1)
        r.range(r.lo, r.hi + 1);                                              // staging.inc:55-57: slid += 1
        r.expect("range grows", 1, true, true, 0, false, false, false);
        r.slide();
        r.expect("slide", 2, true, true, 0, false, false, false);
        for (int i = 0; i < 6; i++) r.slide();
        r.expect("8 appended", 8, true, true, 0, false, false, false);
        r.slide();
        r.expect("9 appended", 0, true, true, 0, false, false, false);        // solve.inc:265: tail <= 8, else a full linearisation
        r.solved();
        r.expect("solve", 0, true, true, 0, false, false, false);
    }
    // a write 1, 8, 9 slots inside the end
    for (int inside : {1, 8, 9}) {
        {   // warm: touch() :25-30 -- redo = inside; beyond 8: cold()
            Rig r = make("late write warm", WARM);
            r.m.stashed(r.lo);
            r.write(0, r.hi - inside);
            r.expect("write", inside <= 8 ? inside : 0, inside <= 8, true, 0, inside <= 8, false, false);
            r.write(0, r.hi);                       // a later append does not shorten the tail (:27 keeps the maximum)
            r.expect("then append", inside <= 8 ? inside : 0, inside <= 8, true, 0, inside <= 8, false, false);
        }
        {   // incremental: touch() :16-19 -- first dirty slot recorded, not warm: return.  appended = hi - first dirty (compat.inc:31-32)
            Rig r = make("late write inc", INC);
            r.write(0, r.hi - inside);
            r.expect("write", 0, false, false, inside, false, false, false);
            r.write(0, r.hi - 2);
            r.expect("second write", 0, false, false, inside > 2 ? inside : 2, false, false, false);
        }
        {   // both: touch() :16-23 -- beyond 8 only the warm flag goes (no cold(): the stash and the panels stay)
            Rig r = make("late write both", BOTH);
            r.m.stashed(r.lo);
            r.write(0, r.hi - inside);
            r.expect("write", inside <= 8 ? inside : 0, inside <= 8, false, inside, true, false, false);
        }
    }
    {   // a write within VF_MAX_BANDWIDTH of lo with a stash alive: touch() :15 voids the stash only
        Rig r = make("write near lo", BOTH);
        r.hi = r.lo + 6;
        r.m.stashed(r.lo);
        r.expect("stashed", 0, true, false, 0, true, false, false);
        r.write(0, r.lo + VF_MAX_BANDWIDTH + 1);
        r.expect("beyond reach", r.hi - (r.lo + VF_MAX_BANDWIDTH + 1), true, false, r.hi - (r.lo + VF_MAX_BANDWIDTH + 1), true, false, false);
        r.write(0, r.lo + VF_MAX_BANDWIDTH);
        r.expect("within reach", r.hi - (r.lo + VF_MAX_BANDWIDTH), true, false, r.hi - (r.lo + VF_MAX_BANDWIDTH), false, false, false);
        r.write(0, r.lo);            // at lo: not behind the first keyframe -> cold() (:30)
        r.expect("at lo", 0, false, true, r.hi - (r.lo + VF_MAX_BANDWIDTH), false, false, false);
    }
    {   // the stash: fits only the keyframe it was made for (window.inc:11), committed once (:16), void after a cold()
        Rig r = make("stash", WARM);
        r.m.stashed(r.lo);
        r.lo++;                      // (drop_oldest moves lo without touching the memory, window.inc:215)
        r.expect("lo moved", 0, true, true, 0, false, false, false);
        r.lo--;
        r.m.stash_committed();
        r.expect("committed", 0, true, true, 0, false, false, false);
        r.m.stashed(r.lo);
        r.solved(false, true);       // a replay leaves it alone (solve.inc:354-356: mark_solved only)
        r.expect("replayed solve", 0, true, true, 0, true, false, false);
        r.solved();                  // a solve whose stages ran voids it (cold() in every stage)
        r.expect("solve", 0, true, true, 0, false, false, false);
    }
    {   // set_range, staging.inc:55-62
        Rig r = make("set_range", BOTH);
        r.m.stashed(r.lo);
        r.range(r.lo, r.hi + 2);                                   // grows: slid += 2, first dirty = old hi
        r.expect("grows", 2, true, false, 2, true, false, false);
        r.range(r.lo, r.hi);                                       // same range: grows (hi >= old hi) by nothing
        r.expect("same", 2, true, false, 2, true, false, false);
        r.range(r.lo, r.hi - 1);                                   // shrinks: cold
        r.expect("shrinks", 0, false, true, 1, false, false, false);     // (first dirty slot stays where the growth put it)
        Rig s = make("set_range lo", BOTH);
        s.range(s.lo + 1, s.hi);                                   // moves lo: cold
        s.expect("moves lo", 0, false, true, 0, false, false, false);
        Rig t = make("set_range inc", INC);
        t.m.stashed(t.lo);
        t.range(t.lo, t.hi + 1);                                   // not warm: cold(), but inc_keeps puts inc_valid back (:56-61)
        t.expect("grows, not warm", 0, false, false, 1, false, false, false);
        Rig u("set_range empty");
        u.lo = u.hi = 0;
        u.solved();
        u.range(0, 5);                                             // from an empty window (:55 old hi > old lo fails): cold
        u.expect("from empty", 0, false, true, 0, false, false, false);
    }
    {   // several windows: nothing is followed (touch :16, :25 and set_range :55 all ask for B == 1); slides still count (window.inc:248)
        Rig r("several windows", false);
        r.updated();
        r.solved(false, true);
        r.slide();
        r.expect("slide", 1, true, false, 1, false, false, false);
        r.write(0, r.hi);
        r.expect("append", 0, false, true, 1, false, false, false);
        r.solved();
        r.range(r.lo, r.hi + 1);
        r.expect("range grows", 0, false, true, 1, false, false, false);
        r.updated();
        r.write(0, r.hi - 1);        // compat.inc:32 B == 1 only: inc_slid alone counts
        r.m.slid_by_one();
        r.expect("inc, several", 0, false, true, 0, false, false, false);
    }
    {   // sharded: warm is recorded but no solve takes a tail (solve.inc:265 sh_G <= 1)
        Rig r("sharded", true, true);
        r.solved();
        r.slide();
        r.expect("slide", 0, true, true, 0, false, false, false);
    }
    {   // far factors alive / cold_start: solve.inc:314
        Rig r("far alive");
        r.solved(true);
        r.slide();
        r.expect("far", 0, false, true, 0, false, false, false);
        Rig s("cold_start", true, false, true);
        s.solved();
        s.slide();
        s.expect("cold_start", 0, false, true, 0, false, false, false);
    }
    {   // predict_from_estimate, compat.inc:94: touch, cold, and inc_valid put back if it was set and the write lies behind lo
        Rig r = make("predict_from_estimate", BOTH);
        r.m.stashed(r.lo);
        r.m.predicted_from_estimate(0, r.hi, r.lo);
        r.expect("behind lo", 0, false, false, 0, false, false, false);
        r.m.predicted_from_estimate(0, r.hi - 3, r.lo);
        r.expect("inside", 0, false, false, 3, false, false, false);
        r.m.predicted_from_estimate(0, r.lo, r.lo);
        r.expect("at lo", 0, false, true, 3, false, false, false);
        Rig s("predict_from_estimate several", false);
        s.updated();
        s.m.predicted_from_estimate(0, s.hi, s.lo);
        s.expect("several windows", 0, false, true, 0, false, false, false);
    }
    {   // incremental update: slides and writes since the last one (compat.inc:31-32), reset by it (:45-46)
        Rig r = make("isam", INC);
        r.slide();
        r.slide();
        r.expect("two slides", 0, false, false, 2, false, false, false);
        r.write(0, r.hi - 5);
        r.expect("late write", 0, false, false, 5, false, false, false);
        if (!r.m.inc_slid()) { failures++; printf("FAIL isam: inc_slid\n"); }
        r.updated();
        r.expect("update", 0, false, false, 0, false, false, false);
        if (r.m.inc_slid()) { failures++; printf("FAIL isam: inc_slid after update\n"); }
        r.m.rewritten();
        r.expect("cold", 0, false, true, 0, false, false, false);
    }
    {   // compact (window.inc:281, :285) and grow (:472-473); covariances (marginals.inc:62 cold, :101)
        Rig r = make("compact / grow", BOTH);
        r.slide();
        r.m.rewritten();
        r.m.covariances_computed();
        r.expect("marginals", 0, false, true, 1, false, false, true);
        r.solved();
        r.expect("solve keeps covariances", 0, true, true, 1, false, false, true);
        r.m.compacted();
        r.expect("compacted", 0, false, true, 1, false, false, false);
        r.solved();
        r.slide();
        r.m.grown();
        r.solved(false, true);       // slid / redo were reset (:473): a replayed solve's successor starts from a tail of 0
        r.expect("grown", 0, true, true, 1, false, false, false);
    }
    {   // what the covariance calls leave: the pose records only with the blocks and the flag of the LAST call, scores only of the
        // records of that call (marginals.inc: pm_on, sc_rows_used and the sig_G / pm_G / sc_G comparisons of the commit "Degeneracy
        // scores of the solved keyframes' pose marginals, on device")
        Rig r = make("covariances", WARM);
        r.expect_cov("solved, never asked", false, false, 0);
        r.m.scores_computed(3);                    // (the engine refuses this call; the account does not depend on that)
        r.expect_cov("scores of nothing", false, false, 0);
        r.m.covariances_started();
        r.m.covariances_computed(true);
        r.expect_cov("marginals with the flag", true, true, 0);
        r.m.scores_computed(0);
        r.m.scores_computed(3);
        r.expect_cov("scores", true, true, 3);
        r.slide();
        r.solved();
        r.expect_cov("a solve keeps all three", true, true, 3);
        r.m.covariances_started();
        r.m.covariances_computed(true);
        r.expect_cov("a covariance call voids the scores", true, true, 0);
        r.m.scores_computed(2);
        r.m.covariances_started();
        r.m.covariances_computed(false);
        r.expect_cov("without the flag: pose records and scores void", true, false, 0);
        r.m.covariances_computed(true);
        r.m.scores_computed(1);
        r.m.covariances_started();                 // ... and the call fails on the way (an allocation, a launch)
        r.expect_cov("started, never computed", false, false, 0);
        r.m.scores_computed(1);
        r.expect_cov("scores of void records", false, false, 0);
        for (int grown = 0; grown < 2; grown++) {
            r.m.covariances_started();
            r.m.covariances_computed(true);
            r.m.scores_computed(3);
            if (grown) r.m.grown();
            else r.m.compacted();
            r.expect_cov(grown ? "grown" : "compacted", false, false, 0);
            r.m.scores_computed(3);
            r.expect_cov(grown ? "grown, scores" : "compacted, scores", false, false, 0);
        }
    }
    {   // the cached result: set at the end of an adaptive solve (solve.inc:308), kept across vf_engine_marginals
        // (marginals.inc:24-26), void after any other entry point (vf_engine.hip:396), vf_engine_read_result included (staging.inc:84-85)
        Rig r = make("result cache", WARM);
        r.m.result_cached(r.hi - 1);
        r.expect("cached", 0, true, true, 0, false, true, false);
        r.m.entry_ran(true);
        r.expect("marginals", 0, true, true, 0, false, true, false);
        bool wrong = r.m.result_cached_for(0, r.hi - 2, false) || r.m.result_cached_for(0, r.hi - 1, true) || r.m.result_cached_for(1, r.hi - 1, false);
        if (wrong) { failures++; printf("FAIL result cache: another slot / the estimate / another window\n"); }
        r.m.entry_ran(false);
        r.expect("any other call", 0, true, true, 0, false, false, false);
        // sticky words an early read consumed are handed on once (solve.inc:291-293, staging.inc:95-97)
        r.m.sticky_consumed(1, 4);
        r.m.sticky_consumed(0, 2);
        int s0 = 0, s1 = 8;
        r.m.sticky_handed_on(&s0, &s1);
        int t0 = 0, t1 = 0;
        r.m.sticky_handed_on(&t0, &t1);
        if (s0 != 1 || s1 != 14 || t0 != 0 || t1 != 0) { failures++; printf("FAIL result cache: sticky words %d %d %d %d\n", s0, s1, t0, t1); }
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("engine_memory ok\n");
    return 0;
}
