"""Scripted engine-level call sequences that exercise what the engine remembers from solve to solve (csrc/vf_engine_memory.hpp):
warm tails, late writes, set_range, several windows, cold_start, marginalise-ahead / commit, the cached result block,
incremental updates, far factors, compact and grow in mid-run, what the covariance calls leave across those two, each with
vf_engine_opts.use_hip_graph off and on where it applies.

After each call one line: the call, its return code, and what the ABI shows -- vf_engine_graph_info, vf_engine_solve_form,
vf_engine_incremental_info, a digest of the window's states and the last state as hex; after a read of covariances, pose
records or scores a digest of what it returned.  Two builds of the library that do the same thing print the same
bytes; under `rocprofv3 --kernel-trace -- python tools/engine_sequences.py` they launch the same kernels in the same order (a warm tail shows as k_linearize_tail, a committed stash as k_marg_commit, a cached result as a
missing k_read_result, a re-capture in graph_info).

    python tools/engine_sequences.py [scenario ...]        (default: all)
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vil_sensor_fusion_amd import Engine, EngineOpts, synth  # noqa: E402
from vil_sensor_fusion_amd._lib import VilFusionError  # noqa: E402
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS  # noqa: E402

SWEEP = dict(chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, refine_iterations=0, lm_excursion=0)


class Run:
    """one engine, window w's range mirrored here; every call goes through call() and prints one line"""

    def __init__(self, name, n_total, lo, n0, windows=1, **opts):
        self.name, self.B = name, windows
        self.eng = Engine(EngineOpts(windows=windows, capacity=n_total, **opts))
        self.seqs = [synth.make_sequence(seed=11 + w, n_kf=n_total) for w in range(windows)]
        self.btw = [synth.between_records(s) for s in self.seqs]
        for w, seq in enumerate(self.seqs):
            e = self.eng
            e.preintegrate(w, 1, seq.imu_off[1:], seq.imu_steps, np.zeros(6), synth.CARLA_IMU_COV)
            e.set_between(w, seq.btw_a, seq.btw_b, self.btw[w])
            e.set_states(w, lo, seq.gt_states[lo:lo + 1])
            e.set_prior(w, lo, synth.prior_record(seq.gt_states[lo], REFERENCE_PRIOR_SIGMAS))
            e.set_range(w, lo, lo + 1)
            e.predict(w, lo + 1, n0 - 1)
            e.set_range(w, lo, lo + n0)
        self.lo, self.hi, self.shift = lo, lo + n0, 0
        print(f"== {name}: {windows} window(s) [{lo}, {lo + n0}) {opts}")

    def show(self, what, rc, probe=True):
        e = self.eng
        line = f"{self.name} | {what} -> {rc}"
        if probe:
            g = e.graph_info()
            line += f" | graph {g} form {e.solve_form()}"
            if self.eng.opts.incremental:
                line += f" inc {e.incremental_info(0)}"
            for w in range(self.B):
                s = e.get_states(w, self.lo, self.hi - self.lo)
                line += f" | w{w} {hashlib.sha256(s.tobytes()).hexdigest()[:16]} {s[-1].tobytes().hex()}"
        print(line, flush=True)

    def call(self, what, fn, *a, probe=True, **k):
        try:
            out, rc = fn(*a, **k), 0
        except VilFusionError as err:
            out, rc = None, err.code
        self.show(what, rc, probe)
        return out

    # ---- the moves of a fixed-lag loop
    def iterate(self, k=3, probe=True):
        self.call(f"iterate({k})", self.eng.iterate, k, probe=probe)

    def slide(self, marginalize=True):
        self.call(f"slide(marginalize={marginalize})", self.eng.slide, REFERENCE_PRIOR_SIGMAS, marginalize, probe=False)
        self.lo, self.hi = self.lo + 1, self.hi + 1

    def rewrite_between(self, w, inside):
        """send again the between records that end `inside` slots in front of the window's end (0: the slot behind the end)"""
        slot = self.hi - inside + self.shift
        seq = self.seqs[w]
        m = seq.btw_b == slot
        self.call(f"set_between(w{w}, b = hi - {inside}, {int(m.sum())} records)", self.eng.set_between, w, seq.btw_a[m] - self.shift, seq.btw_b[m] - self.shift,
                  self.btw[w][m], probe=False)

    def set_range(self, lo, hi):
        self.call(f"set_range({lo - self.lo:+d}, {hi - self.hi:+d})", self.eng.set_range, 0, lo, hi, probe=False)
        self.lo, self.hi = lo, hi


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:16]


def marginals(r, compute=True, far=False):
    """what the covariance calls leave, read back (a digest each): the blocks, the pose records, one set of scores.
    compute=False: only the reads, of whatever the last calls left (after compact / grow: refusals)"""
    e, n = r.eng, r.hi - r.lo
    if compute:
        r.call(f"marginals(far={far}, pose=True)", e.marginals, far, True, probe=False)
    reads = [("read_marginals", lambda: digest(e.read_marginals(0, r.lo, n))),
             ("read_pose_marginals", lambda: digest(*e.read_pose_marginals(0, r.lo, n))),
             ("marginal_scores(d_opt)", lambda: e.marginal_scores("d_opt")),
             ("read_marginal_scores", lambda: digest(*e.read_marginal_scores(0, r.lo, n).values()))]
    for what, fn in reads if compute else reads[:2] + reads[3:]:
        out = r.call(what, fn, probe=False)
        if out:
            print(f"    {out}")


def fixed_lag(graph):
    r = Run(f"fixed_lag graph={int(graph)}", 256, 64, 40, use_hip_graph=graph, **SWEEP)
    r.iterate(3)
    r.iterate(3)                                   # nothing since: a cold solve without a graph, a replay with one
    for inside in (0, 1, 8, 9):                    # late writes in front of the end: the tail grows, beyond 8 the solve is cold
        r.slide()
        r.rewrite_between(0, inside)
        r.iterate(2)
    r.slide(); r.slide()
    r.iterate(3)
    for _ in range(9):
        r.slide()
    r.iterate(2)                                   # nine appended: a full linearisation
    r.slide(marginalize=False)
    r.iterate(2)
    r.call("predict(hi, 1)", r.eng.predict, 0, r.hi, 1, probe=False)
    r.set_range(r.lo, r.hi + 1)                    # append by range
    r.iterate(2)
    r.set_range(r.lo, r.hi)
    r.iterate(1)
    r.set_range(r.lo, r.hi - 1)                    # shrinks: cold
    r.iterate(2)
    r.set_range(r.lo + 1, r.hi)                    # moves lo: cold
    r.iterate(2)
    r.call("set_range(bad)", r.eng.set_range, 0, 5, 4, probe=False)
    r.iterate(1)
    r.slide()
    marginals(r)
    r.call("compact(64)", r.eng.compact, 64, probe=False)
    r.lo, r.hi, r.shift = r.lo - 64, r.hi - 64, 64
    marginals(r, compute=False)
    r.iterate(2)
    marginals(r)
    r.slide()
    r.iterate(2)
    r.slide()
    r.call("grow(512)", r.eng.grow, 512)
    marginals(r, compute=False)
    r.iterate(2)
    r.slide()
    r.iterate(2)
    r.call("marginals", r.eng.marginals, probe=False)
    marginals(r, compute=False)                    # without the flag: the blocks, no pose records, no scores
    marginals(r)
    r.iterate(2)
    r.eng.close()


def several_windows(graph):
    r = Run(f"several_windows graph={int(graph)}", 128, 0, 40, windows=3, use_hip_graph=graph, **SWEEP)
    r.iterate(3)
    r.slide()
    r.iterate(2)
    r.slide()
    r.rewrite_between(0, 0)                        # an append, but `slid` is one count for the whole engine: cold
    r.iterate(2)
    r.eng.close()
    c = Run(f"cold_start graph={int(graph)}", 128, 0, 40, cold_start=True, use_hip_graph=graph, **SWEEP)
    c.iterate(3)
    c.slide()
    c.iterate(2)
    c.eng.close()


def read_result(r, slot, estimate=False):
    out = r.call(f"read_result(hi - {r.hi - slot}, estimate={estimate})", r.eng.read_result, 0, slot, estimate, probe=False)
    if out:
        print(f"    {out['state'].tobytes().hex()} cost {out['cost'].hex()} {out['accepted']} {out['rejected']} {out['solve_failures']} {out['device_flags']}")


def graph_manager(graph):
    """the call pattern of vf_solve: asynchronous staging, termination rule, marginalise ahead behind the solve"""
    r = Run(f"graph_manager graph={int(graph)}", 256, 0, 40, use_hip_graph=graph)
    r.call("set_async", r.eng.set_async, True, probe=False)
    r.call("set_convergence", r.eng.set_convergence, 1e-5, 1e-5, probe=False)
    ahead = r.eng._l.vf_engine_marginalize_ahead
    for step in range(8):
        r.iterate(5, probe=False)
        if step == 2:
            r.call("marginals", r.eng.marginals, probe=False)          # leaves the cached result alone
        if step == 3:
            read_result(r, r.hi - 2)                                   # another slot: read again
        if step == 4:
            read_result(r, r.hi - 1, estimate=True)
        if step == 5:
            r.call("get_states", r.eng.get_states, 0, r.lo, 1, probe=False)     # any other call voids the cache
        read_result(r, r.hi - 1)
        r.call("marginalize_ahead", lambda: ahead(r.eng._h), probe=False)
        r.call("predict(hi, 1)", r.eng.predict, 0, r.hi, 1, probe=False)
        r.rewrite_between(0, 0)
        if step == 6:
            r.rewrite_between(0, r.hi - r.lo - 2)                      # within a factor's reach of lo: the stash is void
        r.call("marginalize", r.eng.marginalize, probe=False)
        r.call("drop_oldest", r.eng.drop_oldest, probe=False)
        r.lo += 1
        r.set_range(r.lo, r.hi + 1)
    r.iterate(5)
    r.eng.close()


def isam(graph):
    del graph
    r = Run("isam", 256, 0, 40, incremental=1, **SWEEP)
    step = lambda: r.call("isam_step", r.eng.isam_step, 1e-4)
    step()
    step()
    for inside in (None, 1, 5):
        r.call("predict_from_estimate(hi, 1)", r.eng.predict_from_estimate, 0, r.hi, 1, probe=False)
        r.set_range(r.lo, r.hi + 1)
        if inside:
            r.rewrite_between(0, inside)
        step()
    r.slide()
    step()
    r.call("predict_from_estimate(lo + 1)", r.eng.predict_from_estimate, 0, r.lo + 1, 1, probe=False)
    step()
    r.call("predict_from_estimate(lo)", r.eng.predict_from_estimate, 0, max(r.lo, 1), 1, probe=False)
    step()
    r.call("set_states", r.eng.set_states, 0, r.hi - 1, r.eng.get_states(0, r.hi - 1, 1), probe=False)
    step()
    r.iterate(2)
    step()
    r.call("grow(512)", r.eng.grow, 512)
    step()
    r.eng.close()


def far(graph):
    r = Run(f"far graph={int(graph)}", 128, 0, 48, use_hip_graph=graph)
    seq = r.seqs[0]
    rec = synth.between_records(seq)[:1].copy()
    r.iterate(3)
    # a far factor 5 -> 40 (any record will do: only the bookkeeping is looked at): while it is alive every solve is cold
    r.call("set_extra_between", r.eng.set_extra_between, 0, np.array([5], dtype=np.int32), np.array([40], dtype=np.int32), rec)
    r.iterate(2)
    r.slide()
    r.iterate(2)
    r.call("marginals", r.eng.marginals, probe=False)         # refused: a far factor is alive
    marginals(r, far=True)
    r.call("grow(256)", r.eng.grow, 256)
    marginals(r, compute=False)
    r.iterate(2)
    marginals(r, far=True)
    r.call("set_shard(0, 2)", r.eng.set_shard, 0, 2, probe=False)
    r.call("iterate on a shard", r.eng.iterate, 1, probe=False)
    r.eng.close()


SCENARIOS = dict(fixed_lag=fixed_lag, several_windows=several_windows, graph_manager=graph_manager, isam=isam, far=far)

if __name__ == "__main__":
    for name in sys.argv[1:] or SCENARIOS:
        for graph in (False, True):
            if name == "isam" and graph:
                continue
            SCENARIOS[name](graph)
    print("engine_sequences done")
