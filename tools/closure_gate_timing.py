#!/usr/bin/env python3
"""What the loop-closure gate costs: vf_engine_gate_closures at --windows x --n keyframes, wall clock around a synchronised call and
the HIP-event time of its kernels (vf_engine_closure_gate_status; the factorisation is in both), median of --reps -- with one
candidate (lo, hi-1) per window and with four, without far factors and with one alive per window.  Beside each figure the time of
vf_engine_marginals_ex at the same shape from the same run (VF_MARGINALS_FAR where a far factor is alive): what a caller would
otherwise have to run, and still not get the block.  Then vf_gate_closure on a handle of --handle-n keyframes, without and with a
closure alive.

Writes JSON (profiles/closure_gate_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 900 python tools/closure_gate_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REC = np.concatenate([[1.0], np.zeros(6), np.triu(np.eye(6) * 100.0)[np.triu_indices(6)]])


def med(x):
    return dict(median=float(np.median(x)), samples=[float(v) for v in x])


def engine_part(windows, n, reps):
    from oracle import oracle
    from tests import helpers
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    from vil_sensor_fusion_amd._lib import check
    oracle.build()
    seq = synth.make_sequence(seed=3, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.0)
    eng = Engine(EngineOpts(windows=windows, capacity=(n + 1 + 63) // 64 * 64))
    for w in range(windows):
        helpers.load_engine(eng, w, prob)
    eng.iterate(2)
    eng.sync()
    lists = {"one_candidate": [(0, n - 1)], "four_candidates": [(0, n - 1), (0, 1), (n - 2, n - 1), (1, n - 2)]}
    out = {}
    for far in (False, True):
        if far:
            for w in range(windows):
                eng.set_extra_between(w, np.array([n // 4], dtype=np.int32), np.array([3 * n // 4], dtype=np.int32), REC[None])

        def marginals():
            eng.sync()
            t0 = time.perf_counter()
            eng.marginals(far=far)
            eng.sync()
            return (time.perf_counter() - t0) * 1e3

        marginals()                      # the first call allocates
        part = dict(marginals_ex_ms=med([marginals() for _ in range(reps)]))
        for name, cands in lists.items():
            ws = np.repeat(np.arange(windows, dtype=np.int32), len(cands))
            a = np.tile(np.array([c[0] for c in cands], dtype=np.int32), windows)
            b = np.tile(np.array([c[1] for c in cands], dtype=np.int32), windows)
            recs = np.tile(REC, (ws.size, 1))

            def gate():
                eng.sync()
                t0 = time.perf_counter()
                check(eng._l.vf_engine_gate_closures(eng._h, int(ws.size), ws.ctypes.data, a.ctypes.data, b.ctypes.data, recs.ctypes.data, 22.46))
                eng._closure_n = int(ws.size)
                eng.sync()
                return (time.perf_counter() - t0) * 1e3, eng.closure_gate_status()[1]
            gate()                       # the first call allocates
            t = np.array([gate() for _ in range(reps)])
            status, nis = eng.read_closure_gate_all(ws.size)
            assert np.all(status == 0) and np.all(np.isfinite(nis))
            part[name] = dict(call_ms=med(t[:, 0]), kernel_ms=med(t[:, 1]), scratch_bytes=eng.closure_gate_status()[2])
        out["one_far_factor_per_window" if far else "no_far_factor"] = part
    eng.close()
    return dict(windows=windows, keyframes=n, **out)


def handle_part(n, reps):
    from vil_sensor_fusion_amd import synth
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    seq = synth.make_sequence(seed=5, n_kf=n + 3, keep_raw=True)
    gm = GraphManager(capacity=(n + 64 + 63) // 64 * 64, iterations=3, lag=0)
    gm.setInitialState(seq.gt_states[0])
    i = 0

    def keyframe(k):
        nonlocal i
        while i < seq.imu_t.size and seq.imu_t[i] <= seq.kf_time[k] + 0.01:
            gm.addIMUMeasurement(seq.imu_t[i], seq.imu_acc[i], seq.imu_gyro[i])
            i += 1
        key = gm.reserveNode(seq.kf_time[k])
        gm.solve()
        return key
    for k in range(1, n):
        key = keyframe(k)
    pose, cov = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)), np.eye(6) * 1e-2

    def call(a, b):
        t0 = time.perf_counter()
        g = gm.gate_closure(a, b, pose, cov, 22.46)
        assert g["status"] == "ok"
        return (time.perf_counter() - t0) * 1e3
    call(2, key)
    out = dict(keyframes=n, no_closure_alive_ms=med([call(2, key) for _ in range(reps)]))
    gm.addBetweenFactor(n // 4, 3 * n // 4, pose, np.eye(6) * 10.0)
    key = keyframe(n)
    call(2, key)
    out["one_closure_alive_ms"] = med([call(2, key) for _ in range(reps)])
    gm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--handle-n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closure_gate_timing.json"))
    a = ap.parse_args()
    res = dict(engine=engine_part(a.windows, a.n, a.reps), handle=handle_part(a.handle_n, a.reps))

    def brief(d):
        return {k: brief(v) for k, v in d.items() if k != "samples"} if isinstance(d, dict) else d
    print(json.dumps(brief(res), indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
