// tests/native/engine_memory_propagate.cpp -- the one fact SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) keeps about
// vf_engine_propagate_tail: a propagation exists, with or without covariance; grown() voids it; nothing else does.
#include <cstdio>

#include "vf_engine_memory.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    vf::SolveMemory m;
    CHECK(!m.propagation_valid() && !m.propagated_covariance_valid());     // a new engine has none
    m.propagated(false);
    CHECK(m.propagation_valid() && !m.propagated_covariance_valid());      // state only
    m.propagated(true);
    CHECK(m.propagation_valid() && m.propagated_covariance_valid());
    m.propagated(false);                                                    // the last call counts
    CHECK(m.propagation_valid() && !m.propagated_covariance_valid());
    m.propagated(true);

    // solves, updates, slides, writes, the covariance calls, compaction: the buffer is the propagation's own, it stays
    m.solve_ended(false, false);
    m.solve_ended(true, true);
    m.inc_update_ended(true);
    m.inc_update_ended(false);
    m.slid_by_one();
    m.rewritten();
    m.written_from(0, 5, 0, 8);
    m.range_set(0, 9, 0, 8);
    m.predicted_from_estimate(0, 8, 0);
    m.stashed(0);
    m.stash_committed();
    m.result_cached(7);
    m.entry_ran(false);
    m.entry_ran(true);
    CHECK(m.propagation_valid() && m.propagated_covariance_valid());
    m.covariances_computed(true);
    m.scores_computed(3);
    m.covariances_started();
    CHECK(!m.covariances_valid());
    CHECK(m.propagation_valid() && m.propagated_covariance_valid());        // covariances_started() voids the marginals, not this
    m.compacted();
    CHECK(m.propagation_valid() && m.propagated_covariance_valid());

    // ... and the propagation touches nothing the other queries report
    vf::SolveMemory a, b;
    for (vf::SolveMemory* s : {&a, &b}) {
        s->solve_ended(false, false);
        s->slid_by_one();
        s->covariances_computed(true);
        s->scores_computed(2);
        s->result_cached(3);
        s->stashed(1);
    }
    b.propagated(true);
    b.entry_ran(true);                                                      // (what the entry point itself reports)
    a.entry_ran(true);
    CHECK(a.tail() == b.tail() && a.is_warm() == b.is_warm() && a.inc_whole_window() == b.inc_whole_window() && a.inc_appended(9) == b.inc_appended(9));
    CHECK(a.stash_fits(1) == b.stash_fits(1) && b.stash_fits(1));
    CHECK(a.result_cached_for(0, 3, false) == b.result_cached_for(0, 3, false) && b.result_cached_for(0, 3, false));
    CHECK(b.covariances_valid() && b.pose_records_valid() && b.score_rows() == 2);

    // grown(): new arrays, the buffer stayed with the old ones
    m.grown();
    CHECK(!m.propagation_valid() && !m.propagated_covariance_valid());
    m.propagated(false);
    CHECK(m.propagation_valid());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("engine_memory_propagate ok\n");
    return 0;
}
