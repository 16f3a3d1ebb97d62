"""Scripted engine-level call sequences that exercise what the engine remembers from solve to solve (csrc/vf_engine_memory.hpp):
warm tails, late writes, set_range, several windows, cold_start, marginalise-ahead / commit, the cached result block,
incremental updates, far factors, compact and grow in mid-run, what the covariance calls leave across those two, each with
vf_engine_opts.use_hip_graph off and on where it applies; and the launches whose View differs from the engine's
(csrc/vf_launch_view.hpp): refined and staged solves, the hybrid K4, factor errors, stage timings, one window's H on demand.

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
            states = [e.get_states(w, self.lo, self.hi - self.lo) for w in range(self.B)]
            if self.B > 4:                         # a large batch: one digest over all windows
                line += f" | all {digest(*states)} trials {digest(np.array([sum(e.read_lm(w)[k] for k in ('accepted', 'rejected')) for w in range(self.B)]))}"
                states = []
            for w, s in enumerate(states):
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


# ---- launches whose View differs from the engine's (csrc/vf_launch_view.hpp): another right-hand side with skip flags, restored
# windows only, the hybrid's gate and active list, one window's K3, every window whatever its `done` flag says
FAR_REC = lambda r: synth.between_records(r.seqs[0])[:1].copy()       # (any record will do: what is compared is two builds)


def show_delta(r, what="read_delta"):
    e, n = r.eng, r.hi - r.lo
    out = r.call(what, lambda: digest(*[e.read_delta(w, r.lo, n) for w in range(r.B)]), probe=False)
    print(f"    {out}")


def refined(graph):
    """refined solves with a far factor alive and excursions allowed: correction solves on (nres, z) that skip the stopped windows,
    the far combine on z, relinearize_restored behind every decision, close_excursions; on a batch engine the Woodbury columns
    one after the other through the same band solve"""
    del graph
    for windows in (1, 3):
        r = Run(f"refined windows={windows}", 128, 0, 56, windows=windows, refine_iterations=2, lm_excursion=2)
        w = windows - 1
        r.call(f"set_extra_between(w{w})", r.eng.set_extra_between, w, np.array([5], dtype=np.int32), np.array([40], dtype=np.int32), FAR_REC(r))
        r.iterate(3)
        show_delta(r)
        for ww in range(windows):
            out = r.call(f"read_refine(w{ww}) / read_excursions", lambda: (r.eng.read_refine(ww), r.eng.read_excursions(ww)), probe=False)
            print(f"    {out}")
        r.call("set_convergence", r.eng.set_convergence, 1e-5, 1e-5, probe=False)
        r.iterate(4)
        show_delta(r)
        r.slide()
        r.iterate(2)
        r.eng.close()


def staged(graph):
    """a chunks=4 engine driven stage by stage as a time-sharded caller drives it (a world of one), plain and with every solve
    refined between refine_begin and refine_end"""
    del graph
    for R in (0, 2):
        r = Run(f"staged refine={R}", 128, 0, 64, chunks=4, refine_iterations=R, lm_excursion=2 if R else 0)
        e = r.eng
        r.call("reset_lambda", e.reset_lambda, probe=False)
        r.call("linearize(0)", e.linearize, 0, probe=False)
        r.call("decide(init)", e.decide, True, probe=False)
        for trial in range(3):
            r.call("assemble", e.assemble, probe=False)
            r.call("solve_local", e.solve_local, probe=False)
            r.call("solve_global", e.solve_global, probe=False)
            show_delta(r)
            if R:
                r.call("refine_begin", e.refine_begin, probe=False)
                for _ in range(e.refine_count()):
                    r.call("solve_local", e.solve_local, probe=False)
                    r.call("solve_global", e.solve_global, probe=False)
                    r.call("refine_step", e.refine_step, probe=False)
                r.call("refine_end", e.refine_end, probe=False)
                show_delta(r)
            r.call("retract", e.retract, probe=False)
            r.call("linearize(1)", e.linearize, 1, probe=False)
            r.call(f"decide (trial {trial})", e.decide, False)
            if trial == 0:
                r.call("set_convergence", e.set_convergence, 1e-5, 1e-5, probe=False)      # (the later trials under the rule)
        r.call("close_excursions", e.close_excursions)
        r.eng.close()


def hybrid(graph):
    """130 short windows under the termination rule, perturbed differently so that they stop at different trials: both forms of K4
    are launched and gate themselves on the number still active, with and without the compacted list, with K3 for all windows
    and for the partitioned half only; then H and g of one converged window on demand"""
    for active_list, asm_min in ((1, 1), (0, 1), (1, 0)):
        r = Run(f"hybrid graph={int(graph)} active_list={active_list} assemble_min={asm_min}", 64, 0, 20, windows=130, chunks=1, use_hip_graph=graph,
                sweep_two_sided_max=0, solve_assemble_min=asm_min, hybrid_threshold=65, hybrid_active_list=active_list,
                refine_iterations=0, lm_excursion=0)
        e, n = r.eng, r.hi - r.lo
        rng = np.random.default_rng(5)
        for w in range(r.B):
            s = e.get_states(w, r.lo, n)
            s[1:, 4:10] += rng.normal(size=(n - 1, 6)) * (1e-4 * 10 ** (w % 4))
            e.set_states(w, r.lo, s)
        r.call("set_convergence", e.set_convergence, 1e-5, 1e-5, probe=False)
        r.iterate(6)
        trials = [sum(e.read_lm(w)[k] for k in ("accepted", "rejected")) for w in range(r.B)]
        print(f"    windows by trials taken: {np.bincount(trials).tolist()}")
        out = r.call("read_normal(w77)", lambda: digest(*e.read_normal(77, r.lo, n)), probe=False)
        print(f"    {out}")
        r.slide()
        r.iterate(4)
        r.eng.close()


def errors(graph):
    """factor errors from what a solve left and after a relinearisation, behind a solve that left `done` flags up; with a far factor
    alive, also across a marginalisation, staged synchronously and asynchronously"""
    del graph

    def read_all(r):
        e, n = r.eng, r.hi - r.lo
        for what, fn in (("read_factor_errors", lambda: digest(*e.read_factor_errors(0, r.lo, n))),
                         ("read_far_errors", lambda: digest(*e.read_far_errors(0))),
                         ("read_consistency", lambda: digest(np.frombuffer(repr(sorted(e.read_consistency(0).items())).encode(), dtype=np.uint8))),
                         ("read_health", lambda: sorted(e.read_health().items()))):
            out = r.call(what, fn, probe=False)
            print(f"    {out}")

    for far_on, async_on in ((False, False), (True, False), (True, True)):
        r = Run(f"errors far={int(far_on)} async={int(async_on)}", 128, 0, 48)
        e = r.eng
        if async_on:
            r.call("set_async", e.set_async, True, probe=False)
        r.call("set_convergence", e.set_convergence, 1e-5, 1e-5, probe=False)
        if far_on:
            r.call("set_extra_between", e.set_extra_between, 0, np.array([0], dtype=np.int32), np.array([40], dtype=np.int32), FAR_REC(r))
        r.iterate(5)
        r.call("factor_errors", e.factor_errors, probe=False)
        read_all(r)
        r.call("factor_errors(relinearize)", e.factor_errors, True)
        read_all(r)
        r.iterate(2)
        r.call("marginalize", e.marginalize, probe=False)          # (the far factor at the window's first keyframe goes into the prior)
        r.call("drop_oldest", e.drop_oldest, probe=False)
        r.lo += 1
        r.call("predict(hi, 1)", e.predict, 0, r.hi, 1, probe=False)
        r.set_range(r.lo, r.hi + 1)
        r.iterate(3)
        r.call("factor_errors", e.factor_errors, probe=False)
        read_all(r)
        r.eng.close()


def stages(graph):
    """vf_engine_time_stage of every stage on a converged engine (the timings are not printed: what each stage left is), then a solve;
    H and g of a window whose solves do not keep them"""
    del graph
    from vil_sensor_fusion_amd.engine import STAGES
    for name, opts in (("partitioned", {}), ("assembling", dict(SWEEP, solve_assemble_min=1))):
        r = Run(f"stages {name}", 128, 0, 48, **opts)
        e, n = r.eng, r.hi - r.lo
        r.call("set_convergence", e.set_convergence, 1e-5, 1e-5, probe=False)
        r.iterate(5)
        for stage in STAGES:
            r.call(f"time_stage({stage})", e.time_stage, stage, 2)
            show_delta(r)
        out = r.call("read_normal", lambda: digest(*e.read_normal(0, r.lo, n)), probe=False)
        print(f"    {out}")
        r.iterate(2)
        out = r.call("read_normal", lambda: digest(*e.read_normal(0, r.lo, n)), probe=False)
        print(f"    {out}")
        r.eng.close()


SCENARIOS = dict(fixed_lag=fixed_lag, several_windows=several_windows, graph_manager=graph_manager, isam=isam, far=far,
                 refined=refined, staged=staged, hybrid=hybrid, errors=errors, stages=stages)
NO_GRAPH = ("isam", "refined", "staged", "errors", "stages")        # scenarios that have no replayed form

if __name__ == "__main__":
    for name in sys.argv[1:] or SCENARIOS:
        for graph in (False, True):
            if name in NO_GRAPH and graph:
                continue
            SCENARIOS[name](graph)
    print("engine_sequences done")
