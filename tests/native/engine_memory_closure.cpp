// tests/native/engine_memory_closure.cpp -- the fact SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) keeps for the
// loop-closure gate: how many records the last vf_engine_gate_closures left to be read (closure_gated / closure_gate_count: of the
// call that wrote them, later solves leave them, a compacted or grown engine loses them, a call that is let in voids the last
// one's from its start).
#include <cstdio>

#include "vf_engine_memory.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    {   // the records
        vf::SolveMemory m;
        CHECK(m.closure_gate_count() == 0);                           // a new engine holds none
        m.solve_ended(false, false);
        CHECK(m.closure_gate_count() == 0);
        m.closure_gated(3);
        CHECK(m.closure_gate_count() == 3);
        // ... are of the call that wrote them: solves, writes, slides, range changes, covariances, propagations, errors and the tail
        // gate leave them
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
        m.gated();
        m.entry_ran(false);
        CHECK(m.closure_gate_count() == 3);
        // ... and the next call replaces them: none while it runs (its buffers may be regrown), then its own
        m.closure_gated(0);
        CHECK(m.closure_gate_count() == 0);
        m.closure_gated(5);
        CHECK(m.closure_gate_count() == 5);
        vf::SolveMemory c = m, g = m;
        c.compacted();
        CHECK(c.closure_gate_count() == 0 && !c.gate_valid() && c.propagation_valid());
        g.grown();
        CHECK(g.closure_gate_count() == 0 && !g.gate_valid() && !g.propagation_valid());
        g.closure_gated(1);
        CHECK(g.closure_gate_count() == 1);
    }
    {   // closure_gated() touches nothing else: what the call does to the savings it says through rewritten() and residuals_current()
        vf::SolveMemory m;
        m.solve_ended(false, false);
        m.stashed(0);
        m.result_cached(7);
        m.entry_ran(true);
        m.covariances_started(), m.covariances_computed_tail();
        m.gated();
        const int tail = m.tail();
        m.closure_gated(4);
        CHECK(m.is_warm() && m.tail() == tail && m.stash_fits(0) && m.result_cached_for(0, 7, false) && m.residuals_vouched());
        CHECK(m.covariances_valid() && m.covariances_tail_only() && m.gate_valid() && !m.propagation_valid() && !m.errors_valid());
    }
    {   // the call as the engine makes it: entry (leaves the result), rewritten(), residuals_current(), closure_gated(n)
        vf::SolveMemory m;
        m.solve_ended(false, false);
        m.result_cached(2);
        m.covariances_started(), m.covariances_computed(true);
        m.entry_ran(true);
        m.closure_gated(0);
        m.rewritten();
        m.residuals_current();
        m.closure_gated(2);
        CHECK(!m.is_warm() && m.tail() == 0);                                      // the engine is left cold
        CHECK(m.residuals_vouched());                                              // every factor was linearised at the current states
        CHECK(m.result_cached_for(0, 2, false));                                   // the result block is as it was
        CHECK(m.covariances_valid() && m.pose_records_valid());                    // sig and its validity are as they were
        CHECK(m.closure_gate_count() == 2);
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("engine_memory_closure ok\n");
    return 0;
}
