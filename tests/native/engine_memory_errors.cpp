// tests/native/engine_memory_errors.cpp -- the fact SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) keeps for
// vf_engine_factor_errors: are the current buffer's residuals those of the current states (residuals_vouched)?  Set by a solve, a
// finished linearisation and the covariances; kept across a write at or beyond the window's end; cleared by every event that
// writes states, records inside the window, ranges or arrays; never set where excursions or incremental updates are on.  And the
// validity of the errors a call left (errors_valid), which only compaction and growth void.
#include <cstdio>

#include "vf_engine_memory.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

// a one-window engine, window [0, 8), just solved
static vf::SolveMemory solved() {
    vf::SolveMemory m;
    m.solve_ended(false, false);
    return m;
}

int main() {
    {
        vf::SolveMemory m;
        CHECK(!m.residuals_vouched() && !m.errors_valid());          // a new engine vouches for nothing and holds no errors
        m.solve_ended(false, false);
        CHECK(m.residuals_vouched());
        m.rewritten();
        CHECK(!m.residuals_vouched());
        m.solve_ended(true, true);                                    // far factors alive, a hipGraph replay: a solve all the same
        CHECK(m.residuals_vouched());
        m.rewritten();
        m.residuals_current();                                        // a finished vf_engine_linearize(e, 0) / vf_engine_isam_step
        CHECK(m.residuals_vouched());
    }
    // an append: records at or beyond the end of the one window (vf_reserve_node preintegrates the next keyframe's record there)
    {
        vf::SolveMemory m = solved();
        m.written_from(0, 8, 0, 8);
        CHECK(m.residuals_vouched());
        m.written_from(0, 11, 0, 8);
        CHECK(m.residuals_vouched());
        m.written_from(0, 7, 0, 8);                                   // the window's last keyframe: inside
        CHECK(!m.residuals_vouched());
    }
    {
        vf::SolveMemory m = solved();
        m.solve_ended(true, false);                                   // not warm (far factors): the append is followed all the same
        CHECK(!m.is_warm());
        m.written_from(0, 8, 0, 8);
        CHECK(m.residuals_vouched());
        m.written_from(0, 3, 0, 8);
        CHECK(!m.residuals_vouched());
    }
    {
        vf::SolveMemory m = solved();                                 // engines of several windows: `hi` is window 0's, nothing is followed
        m.one_window = false;
        m.written_from(1, 8, 0, 8);
        CHECK(!m.residuals_vouched());
        m.solve_ended(false, false);
        m.written_from(0, 8, 0, 8);
        CHECK(!m.residuals_vouched());
    }
    // every event that writes states, records inside [lo, hi), ranges or arrays
    { vf::SolveMemory m = solved(); m.rewritten(); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.range_set(0, 9, 0, 8); CHECK(!m.residuals_vouched()); }       // even the append of a keyframe: it has factors
    { vf::SolveMemory m = solved(); m.range_set(2, 8, 0, 8); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.slid_by_one(); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.predicted_from_estimate(0, 8, 0); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.predicted_from_estimate(0, 3, 0); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.compacted(); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.grown(); CHECK(!m.residuals_vouched()); }
    { vf::SolveMemory m = solved(); m.inc_update_ended(true); CHECK(!m.residuals_vouched()); }
    // ... and what does not: reads, the stash, the cached result, propagation, scores
    {
        vf::SolveMemory m = solved();
        m.entry_ran(true);
        m.entry_ran(false);
        m.stashed(0);
        m.stash_committed();
        m.result_cached(7);
        m.sticky_consumed(1, 2);
        m.propagated(true);
        m.covariances_started();
        m.scores_computed(2);
        m.errors_started();
        m.errors_computed();
        CHECK(m.residuals_vouched());
    }
    // the covariances linearise every factor at the current states: they set it again
    {
        vf::SolveMemory m = solved();
        m.slid_by_one();
        CHECK(!m.residuals_vouched());
        m.covariances_started();
        m.rewritten();
        m.covariances_computed(true);
        CHECK(m.residuals_vouched());
    }
    // never where trials may restore states without their residuals, or where an update linearises a suffix only
    for (int which = 0; which < 2; which++) {
        vf::SolveMemory m;
        (which ? m.incremental : m.excursions) = true;
        m.solve_ended(false, false);
        CHECK(!m.residuals_vouched());
        m.residuals_current();
        CHECK(!m.residuals_vouched());
        m.covariances_computed(false);
        CHECK(!m.residuals_vouched());
        m.inc_update_ended(true);
        CHECK(!m.residuals_vouched());
    }
    {
        vf::SolveMemory m = solved();                                 // switched on after the solve (a window outgrew refine_min_keyframes)
        m.excursions = true;
        CHECK(!m.residuals_vouched());
    }
    // the errors a call left: later solves, slides and writes leave them; compaction and growth void them
    {
        vf::SolveMemory m = solved();
        m.errors_started();
        CHECK(!m.errors_valid());
        m.errors_computed();
        CHECK(m.errors_valid());
        m.solve_ended(false, false);
        m.slid_by_one();
        m.rewritten();
        m.range_set(0, 9, 0, 8);
        m.written_from(0, 2, 0, 9);
        m.predicted_from_estimate(0, 9, 0);
        m.inc_update_ended(false);
        m.covariances_started();
        m.covariances_computed(false);
        CHECK(m.errors_valid());
        m.compacted();
        CHECK(!m.errors_valid());
        m.errors_computed();
        m.grown();
        CHECK(!m.errors_valid());
    }
    // the new fact changes nothing the other queries report
    {
        vf::SolveMemory a, b;
        for (vf::SolveMemory* s : {&a, &b}) {
            s->solve_ended(false, false);
            s->slid_by_one();
            s->written_from(0, 9, 1, 9);
            s->covariances_computed(true);
            s->scores_computed(2);
            s->result_cached(3);
            s->stashed(1);
        }
        b.errors_started();
        b.errors_computed();
        b.residuals_current();
        CHECK(a.tail() == b.tail() && a.tail() == 1 && a.is_warm() == b.is_warm() && a.inc_whole_window() == b.inc_whole_window());
        CHECK(a.stash_fits(1) == b.stash_fits(1) && b.stash_fits(1));
        CHECK(b.result_cached_for(0, 3, false) && b.covariances_valid() && b.pose_records_valid() && b.score_rows() == 2);
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("engine_memory_errors ok\n");
    return 0;
}
