// tests/native/engine_memory_gate.cpp -- the two facts SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) keeps for the
// innovation gate: whether a gate result is there to be read (gated / gate_valid: of the call that wrote it, later solves leave it,
// a compacted or grown engine loses it), and whether the covariances are those of the windows' tails only
// (covariances_computed_tail / covariances_tail_only: valid covariances, no pose records, replaced by the next full call).
#include <cstdio>

#include "vf_engine_memory.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    {   // the gate's result
        vf::SolveMemory m;
        CHECK(!m.gate_valid());                                       // a new engine holds none
        m.solve_ended(false, false);
        m.covariances_started(), m.covariances_computed_tail();
        CHECK(!m.gate_valid());
        m.gated();
        CHECK(m.gate_valid());
        // ... is of the call that wrote it: solves, writes, slides, range changes, new covariances, propagations and errors leave it
        m.rewritten();
        m.written_from(0, 3, 0, 8);
        m.range_set(0, 9, 0, 8);
        m.slid_by_one();
        m.solve_ended(true, true);
        m.inc_update_ended(true);
        m.predicted_from_estimate(0, 8, 0);
        m.covariances_started(), m.covariances_computed(true);
        m.propagated(true);
        m.errors_started(), m.errors_computed();
        m.entry_ran(false);
        CHECK(m.gate_valid());
        // ... and leaves them: the gate fires no other event
        CHECK(m.covariances_valid() && m.pose_records_valid() && m.propagated_covariance_valid() && m.errors_valid());
        vf::SolveMemory c = m, g = m;
        c.compacted();
        CHECK(!c.gate_valid() && !c.covariances_valid() && c.propagation_valid());
        g.grown();
        CHECK(!g.gate_valid() && !g.covariances_valid() && !g.propagation_valid());
        g.gated();
        CHECK(g.gate_valid());
    }
    {   // gated() touches nothing else
        vf::SolveMemory m;
        m.solve_ended(false, false);
        m.stashed(0);
        m.result_cached(7);
        m.entry_ran(true);
        const int tail = m.tail();
        m.gated();
        CHECK(m.is_warm() && m.tail() == tail && m.stash_fits(0) && m.result_cached_for(0, 7, false) && m.residuals_vouched());
        CHECK(!m.covariances_valid() && !m.propagation_valid() && !m.errors_valid());
    }
    {   // tail-only covariances
        vf::SolveMemory m;
        CHECK(!m.covariances_tail_only());
        m.solve_ended(false, false);
        m.covariances_started();
        CHECK(!m.covariances_valid() && !m.covariances_tail_only());
        m.covariances_computed_tail();
        CHECK(m.covariances_valid() && m.covariances_tail_only());
        CHECK(!m.pose_records_valid() && m.score_rows() == 0);       // no records of every keyframe, hence no scores
        CHECK(m.residuals_vouched());                                 // the call linearised every factor, as the full one does
        m.solve_ended(false, false);                                  // a solve leaves covariances as they are, tail or not
        CHECK(m.covariances_valid() && m.covariances_tail_only());
        m.covariances_started();                                      // the next call voids them from its start
        CHECK(!m.covariances_valid() && !m.covariances_tail_only());
        m.covariances_computed(true);                                 // ... and a full one is full
        CHECK(m.covariances_valid() && !m.covariances_tail_only() && m.pose_records_valid());
        m.covariances_started(), m.covariances_computed_tail();       // a tail call after a full one: the pose records are gone
        CHECK(m.covariances_tail_only() && !m.pose_records_valid());
        vf::SolveMemory c = m, g = m;
        c.compacted();
        CHECK(!c.covariances_valid() && !c.covariances_tail_only());
        g.grown();
        CHECK(!g.covariances_valid() && !g.covariances_tail_only());
        m.covariances_started(), m.covariances_computed();            // the plain vf_engine_marginals
        CHECK(m.covariances_valid() && !m.covariances_tail_only() && !m.pose_records_valid());
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("engine_memory_gate ok\n");
    return 0;
}
