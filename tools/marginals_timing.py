#!/usr/bin/env python3
"""vf_engine_marginals timed: host wall time of the call plus a stream synchronisation (median of --reps), at 1 024 windows x
1 000 keyframes (the bench shape; assembling forward sweep + k_band_selinv) and at one window of 1 000 keyframes (the handle's
engine: a single-wave forward sweep + k_band_selinv).  Every window holds the same seeded synthetic problem.  Compares the
batch figure with the HBM floor of the selected inversion (panel read + Sigma write).  Writes JSON (profiles/marginals_timing.json
by default).  Run from the repo root on a GPU box:

    timeout -k 10 900 python tools/marginals_timing.py

and for the per-kernel split, in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o marg -- python tools/marginals_timing.py --reps 2 --out <dir>/t.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(windows, n, chunks):
    from oracle import oracle
    from tests import helpers
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    oracle.build()
    seq = synth.make_sequence(seed=3, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.0)
    eng = Engine(EngineOpts(windows=windows, capacity=(n + 63) // 64 * 64, chunks=chunks))
    for w in range(windows):
        helpers.load_engine(eng, w, prob)
    eng.iterate(2)
    return eng


def time_marginals(eng, reps):
    eng.marginals()                  # first call allocates
    eng.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.marginals()
        eng.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals_timing.json"))
    a = ap.parse_args()
    res = {}
    eng = load(1, a.n, 0)
    res["one_window"] = dict(windows=1, keyframes=a.n, form=eng.solve_form(), ms=time_marginals(eng, a.reps))
    eng.close()
    eng = load(a.windows, a.n, 0)
    med, all_ = time_marginals(eng, a.reps)
    slots = a.windows * a.n
    floor_bytes = slots * (42 * 15 + 120 + 225) * 8
    res["batch"] = dict(windows=a.windows, keyframes=a.n, form=eng.solve_form(), ms=(med, all_),
                        selinv_hbm_bytes=floor_bytes, selinv_hbm_floor_ms_at_8TBps=floor_bytes / 8e12 * 1e3)
    eng.close()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
