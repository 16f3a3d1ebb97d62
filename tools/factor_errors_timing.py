#!/usr/bin/env python3
"""What vf_engine_factor_errors costs on the reuse path: the HIP-event time of one call's launches (k_factor_errors over every window
+ k_batch_health) at the headline batch, 1 024 windows x 1 000 keyframes, median of --reps single calls.  Beside it, as the yardstick,
VF_STAGE_DECIDE of the same engine (k_decide, init form: it reads the same residual bytes and writes one double per window).

The engine is put on the default stream so that events recorded there bracket the call; the residuals are vouched for by a
vf_engine_linearize(e, 0), so the call launches its two kernels and nothing else.

Writes JSON (profiles/factor_errors_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 600 python tools/factor_errors_timing.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_errors_timing.json"))
    a = ap.parse_args()
    import torch
    from vil_sensor_fusion_amd import CHI2_999, Engine, EngineOpts, synth
    from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS
    B, n = a.windows, a.n
    seq = synth.make_sequence(seed=3, n_kf=n)
    eng = Engine(EngineOpts(windows=B, capacity=(n + 63) // 64 * 64))
    btw = synth.between_records(seq)
    for w in range(B):
        eng.preintegrate(w, 1, seq.imu_off[1:], seq.imu_steps, np.zeros(6), synth.CARLA_IMU_COV)
        eng.set_between(w, seq.btw_a, seq.btw_b, btw)
        eng.set_states(w, 0, seq.gt_states[:1])
        eng.set_prior(w, 0, synth.prior_record(seq.gt_states[0], REFERENCE_PRIOR_SIGMAS))
        eng.set_range(w, 0, 1)
    eng.predict(-1, 1, n - 1)
    for w in range(B):
        eng.set_range(w, 0, n)
    eng.set_stream(0)
    torch.cuda.synchronize()
    eng.linearize(0)
    eng.factor_errors(thresholds=CHI2_999)        # the first call allocates
    eng.sync()
    samples = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.factor_errors(thresholds=CHI2_999)
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1))
    health = eng.read_health()
    c = eng.read_consistency(B - 1)
    decide_ms = eng.time_stage("decide", reps=10)           # (a stage call: the engine is cold afterwards)
    counts = eng.counts()
    eng.close()
    kf = B * n
    ms = float(np.median(samples))
    res = dict(windows=B, keyframes=n, factors=dict(imu=counts["imu"], between=counts["between"]),
               bytes_per_keyframe=184, bytes_moved=184 * kf,
               factor_errors=dict(ms=ms, samples=samples, gb_per_s=184 * kf / (ms * 1e-3) / 1e9,
                                  what="one vf_engine_factor_errors(flags = 0): k_factor_errors + k_batch_health, HIP events around the call"),
               decide=dict(ms=decide_ms, what="VF_STAGE_DECIDE, vf_engine_time_stage, mean of 10 launches"),
               factor_errors_over_decide=ms / decide_ms if decide_ms > 0 else None,
               note="the residuals were written by the linearisation just before and the nine calls read the same 0.17 GB, which the 256 MB Infinity Cache holds: a time with warm caches, as inside a solve loop, not an HBM-bound one",
               last_window=dict(total=c["total"], rows=c["rows"], unknowns=c["unknowns"], flagged_imu=c["imu"]["flagged"]), health=health)
    print(json.dumps({k: v for k, v in res.items() if k != "health"}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
