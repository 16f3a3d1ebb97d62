#!/usr/bin/env python3
"""What the innovation gate costs: HIP-event times of vf_engine_gate_tail's pinned copy and of k_gate_between
(vf_engine_gate_status) at --windows x --n keyframes with 10 IMU steps per window (median of --reps); the tail-only marginals
(VF_MARGINALS_TAIL) against the full call at that shape, wall clock around a synchronised call; and the latency of vf_gate_between
on a handle of --handle-n keyframes (the first call, which computes the tail-only covariances, and the calls after it).

Writes JSON (profiles/gate_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 900 python tools/gate_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 10


def engine_part(windows, n, reps):
    from oracle import oracle
    from tests import helpers
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    oracle.build()
    seq = synth.make_sequence(seed=3, n_kf=n + 2)
    prob = helpers.build_problem(oracle, seq, perturb=0.0)
    eng = Engine(EngineOpts(windows=windows, capacity=(n + 1 + 63) // 64 * 64))
    for w in range(windows):
        helpers.load_engine(eng, w, prob, hi=n)
    eng.iterate(2)
    eng.sync()
    st = seq.imu_steps[seq.imu_off[n]:seq.imu_off[n] + STEPS]
    off = (np.arange(windows + 1) * STEPS).astype(np.int32)
    steps = np.tile(st, (windows, 1))
    cov = synth.CARLA_IMU_COV

    def marginals(tail):
        eng.sync()
        t0 = time.perf_counter()
        eng.marginals(tail=tail)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    marginals(False)                     # first call allocates
    full = [marginals(False) for _ in range(max(3, reps // 3))]
    tail = [marginals(True) for _ in range(max(3, reps // 3))]
    rec = np.tile(np.concatenate([[1.0], np.zeros(6), np.triu(np.eye(6) * 100.0)[np.triu_indices(6)]]), (windows, 1))
    out = {}
    for name, a in (("a_is_last", n - 1), ("a_is_before_last", n - 2)):
        aa = np.full(windows, a, dtype=np.int32)

        def gate():
            eng.gate_tail(off, steps, cov, aa, rec, threshold=22.46)
            return eng.gate_status()
        gate()
        t = np.array([gate() for _ in range(reps)])
        status, nis = eng.read_gate_all()
        assert np.all(status == 0) and np.all(np.isfinite(nis))
        out[name] = dict(h2d_ms=float(np.median(t[:, 0])), kernel_ms=float(np.median(t[:, 1])), samples=t.tolist())
    eng.close()
    return dict(windows=windows, keyframes=n, steps_per_window=STEPS, bytes_copied=int(off.nbytes * 3 + rec.nbytes + steps.nbytes), gate=out,
                marginals_full_ms=dict(median=float(np.median(full)), samples=full), marginals_tail_ms=dict(median=float(np.median(tail)), samples=tail))


def handle_part(n, reps):
    from vil_sensor_fusion_amd import synth
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    seq = synth.make_sequence(seed=5, n_kf=n + 3, keep_raw=True)
    gm = GraphManager(capacity=(n + 64 + 63) // 64 * 64, iterations=3, lag=0)
    gm.setInitialState(seq.gt_states[0])
    i = 0

    def keyframe(k, solve):
        nonlocal i
        while i < seq.imu_t.size and seq.imu_t[i] <= seq.kf_time[k] + 0.01:
            gm.addIMUMeasurement(seq.imu_t[i], seq.imu_acc[i], seq.imu_gyro[i])
            i += 1
        key = gm.reserveNode(seq.kf_time[k])
        if solve:
            gm.solve()
        return key
    for k in range(1, n):
        keyframe(k, True)
    key = keyframe(n, False)
    pose, cov = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)), np.eye(6) * 1e-4

    def call():
        t0 = time.perf_counter()
        g = gm.gate_between(key - 1, key, pose, cov, 22.46)
        return (time.perf_counter() - t0) * 1e3, g
    first, g = call()
    assert g["status"] == "ok"
    later = [call()[0] for _ in range(reps)]
    gm.close()
    return dict(keyframes=n, first_call_ms=first, first_call_includes="tail-only marginals of the window (linearise, factorise, two steps of the selected inversion)",
                later_calls_ms=dict(median=float(np.median(later)), samples=later))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--handle-n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_timing.json"))
    a = ap.parse_args()
    res = dict(engine=engine_part(a.windows, a.n, a.reps), handle=handle_part(a.handle_n, a.reps))
    brief = json.loads(json.dumps(res))
    for d in (brief["engine"]["gate"]["a_is_last"], brief["engine"]["gate"]["a_is_before_last"], brief["engine"]["marginals_full_ms"],
              brief["engine"]["marginals_tail_ms"], brief["handle"]["later_calls_ms"]):
        d.pop("samples")
    print(json.dumps(brief, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
