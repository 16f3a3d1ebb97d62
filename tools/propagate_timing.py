#!/usr/bin/env python3
"""What vf_engine_propagate_tail costs: HIP-event times of its pinned copy and of k_propagate (vf_engine_propagate_status), at 1, 64
and 1 024 windows x 10 IMU steps, with the covariance and state-only (median of --reps).  Beside them, as the yardstick, K0's ingest
launch on the same batch (vf_engine_ingest_tail / vf_engine_ingest_status): the same integration plus a reverse Cholesky, without the
prediction and the covariance products.

Writes JSON (profiles/propagate_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 600 python tools/propagate_timing.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 10


def load(windows, n):
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
    eng.marginals()
    eng.sync()
    return eng, seq.imu_steps[seq.imu_off[n]:seq.imu_off[n] + STEPS]


def median_of(fn, reps):
    fn()                                 # first call allocates
    t = np.array([fn() for _ in range(reps)])
    return [float(x) for x in np.median(t, axis=0)], t.tolist()


def measure(windows, n, reps):
    from vil_sensor_fusion_amd import synth
    eng, st = load(windows, n)
    assert st.shape[0] == STEPS
    off = (np.arange(windows + 1) * STEPS).astype(np.int32)
    steps = np.tile(st, (windows, 1))
    cov = synth.CARLA_IMU_COV
    a, rec = np.full(windows, -1, dtype=np.int32), np.zeros((windows, 28))

    def propagate(with_cov):
        eng.propagate_tail(off, steps, cov, covariance=with_cov)
        return eng.propagate_status()

    def ingest():
        eng.ingest_tail(off, steps, cov, a, rec)
        return eng.ingest_status()

    full, full_all = median_of(lambda: propagate(True), reps)
    state, state_all = median_of(lambda: propagate(False), reps)
    k0, k0_all = median_of(ingest, reps)
    assert np.all(np.isfinite(eng.read_propagated(windows - 1)))
    eng.close()
    return dict(windows=windows, keyframes=n, steps_per_window=STEPS, bytes_copied=int(off.nbytes + steps.nbytes),
                propagate=dict(h2d_ms=full[0], kernel_ms=full[1], samples=full_all),
                propagate_state_only=dict(h2d_ms=state[0], kernel_ms=state[1], samples=state_all),
                ingest_tail_k0=dict(h2d_ms=k0[0], kernel_ms=k0[1], samples=k0_all),
                kernel_over_k0=full[1] / k0[1] if k0[1] > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagate_timing.json"))
    a = ap.parse_args()
    res = {f"windows_{w}": measure(w, a.n, a.reps) for w in a.windows}
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk not in ("propagate", "propagate_state_only", "ingest_tail_k0")} |
                      {kk: {x: v[kk][x] for x in ("h2d_ms", "kernel_ms")} for kk in ("propagate", "propagate_state_only", "ingest_tail_k0")}
                      for k, v in res.items()}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
