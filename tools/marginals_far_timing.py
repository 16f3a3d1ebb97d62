#!/usr/bin/env python3
"""vf_engine_marginals_ex(VF_MARGINALS_FAR) timed against the band-only call: host wall time of the call plus a stream
synchronisation (median of --reps).  One window of 1 000 keyframes (the shape of a handle at lag 1 000) with 1, 8 and 32 loop
closures alive (an engine made with max_far_factors = 32), and 1 024 windows x 1 000 keyframes with one far factor per window.
The band-only figure is the same engine without far factors (vf_engine_marginals refuses while any is alive); the difference
is what the downdate adds.  Writes JSON (profiles/marginals_far_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 900 python tools/marginals_far_timing.py

and for the per-kernel split, in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o margfar -- python tools/marginals_far_timing.py --reps 2 --out <dir>/t.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def closure_record(seq, a, b):
    from vil_sensor_fusion_amd import synth
    Ra, Rb = synth.quat_to_rot(seq.gt_states[a, :4]), synth.quat_to_rot(seq.gt_states[b, :4])
    rec = np.zeros(28)
    rec[0:4] = synth.rot_to_quat(Ra.T @ Rb)
    rec[4:7] = Ra.T @ (seq.gt_states[b, 4:7] - seq.gt_states[a, 4:7])
    iu = np.triu_indices(6)
    rec[7 + np.nonzero(iu[0] == iu[1])[0]] = 1.0 / np.sqrt(0.05)
    return rec


def load(windows, n, closures):
    from oracle import oracle
    from tests import helpers
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    oracle.build()
    seq = synth.make_sequence(seed=3, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.0)
    eng = Engine(EngineOpts(windows=windows, capacity=(n + 63) // 64 * 64, max_far_factors=32))
    pairs = [(20 + 25 * i, 80 + 25 * i) for i in range(closures)]
    for w in range(windows):
        helpers.load_engine(eng, w, prob)
        if pairs:
            eng.set_extra_between(w, np.array([a for a, _ in pairs], dtype=np.int32), np.array([b for _, b in pairs], dtype=np.int32),
                                  np.stack([closure_record(seq, a, b) for a, b in pairs]))
    eng.iterate(2)
    return eng


def time_call(eng, far, reps):
    eng.marginals(far=far)           # first call allocates
    eng.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.marginals(far=far)
        eng.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals_far_timing.json"))
    a = ap.parse_args()
    res = {}
    eng = load(1, a.n, 0)
    band1 = time_call(eng, False, a.reps)
    eng.close()
    res["one_window_band_only"] = dict(windows=1, keyframes=a.n, ms=band1)
    for c in (1, 8, 32):
        eng = load(1, a.n, c)
        far = time_call(eng, True, a.reps)
        eng.close()
        res[f"one_window_{c}_closures"] = dict(windows=1, keyframes=a.n, closures=c, m=6 * c, ms=far, added_ms=far[0] - band1[0])
    eng = load(a.windows, a.n, 0)
    bandb = time_call(eng, False, a.reps)
    eng.close()
    eng = load(a.windows, a.n, 1)
    farb = time_call(eng, True, a.reps)
    eng.close()
    res["batch_band_only"] = dict(windows=a.windows, keyframes=a.n, ms=bandb)
    res["batch_1_far_factor_per_window"] = dict(windows=a.windows, keyframes=a.n, closures=1, ms=farb, added_ms=farb[0] - bandb[0])
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
