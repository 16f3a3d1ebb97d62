#!/usr/bin/env python3
"""What VF_MARGINALS_POSE and vf_engine_marginal_scores cost, and what the host route they replace costs: host wall time of the
calls including the synchronisation (median of --reps), at 1 024 windows x 1 000 keyframes and at one window of 1 000.

  marginals            vf_engine_marginals + sync
  marginals_pose       vf_engine_marginals_ex(VF_MARGINALS_POSE) + sync; added_ms = the median difference of alternating calls: the
                       extraction kernel (kernels/kpose.inc); added_resolved says whether it exceeds the spread of the call's own
                       timings (device_route_ms counts it only then).  Its algorithmic traffic is 168 B of each covariance slot + 56 B of state read and
                       624 B written per keyframe: hbm_fraction = those bytes / added time / 8 TB/s
  scores_and_read      vf_engine_marginal_scores(d_opt, all | trans | rot) + vf_engine_read_marginal_scores of ONE window
  host_route           what a caller had to do without them, for EVERY window: vf_engine_read_marginals and vf_engine_get_states,
                       the rotation and permutation of covariance.ros_pose_covariance in numpy (vectorised over the window), and
                       one vf_degeneracy_scores_batch per window (a series must not run across windows).  At the batch it is
                       measured on --host-windows windows and scaled to all of them (scaled_from says so).

Writes JSON (profiles/pose_marginals_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 900 python tools/pose_marginals_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
BYTES_PER_KEYFRAME = 168 + 56 + 624


def load(windows, n):
    from oracle import oracle
    from tests import helpers
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    oracle.build()
    seq = synth.make_sequence(seed=3, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.0)
    eng = Engine(EngineOpts(windows=windows, capacity=(n + 63) // 64 * 64))
    for w in range(windows):
        helpers.load_engine(eng, w, prob)
    eng.iterate(2)
    return eng


def median_ms(fn, reps):
    fn()                                 # first call allocates
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def host_scores(eng, w, n):
    """the parent's only route for one window; returns the d_opt scores of (all, trans, rot)"""
    from vil_sensor_fusion_amd import degeneracy
    S = eng.read_marginals(w, 0, n)[:, :6, :6]
    st = eng.get_states(w, 0, n)
    q = st[:, :4] / np.linalg.norm(st[:, :4], axis=1, keepdims=True)
    qw, qx, qy, qz = q.T
    R = np.empty((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)
    A = np.zeros((n, 6, 6))              # diag(R, R) P, P the swap [omega, v] -> [v, omega]
    A[:, 0:3, 3:6] = R
    A[:, 3:6, 0:3] = R
    cov = A @ S @ A.transpose(0, 2, 1)
    return degeneracy.scores(np.ascontiguousarray(cov.transpose(1, 2, 0)), None, "d_opt")


def measure(windows, n, reps, host_windows):
    eng = load(windows, n)

    def plain():
        eng.marginals()
        eng.sync()

    def pose():
        eng.marginals(pose=True)
        eng.sync()

    def scores():
        eng.marginal_scores("d_opt", ("all", "trans", "rot"))
        return eng.read_marginal_scores(0, 0, n)

    def host():
        for w in range(hw):
            host_scores(eng, w, n)

    hw = min(windows, host_windows)
    plain(), pose()                      # first calls allocate
    ta, tb = [], []
    for _ in range(reps):                # alternating, so that a drift of the 13-18 ms call does not pass for the 0.0-0.2 ms added
        for fn, t in ((plain, ta), (pose, tb)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    a, b = (float(np.median(ta)), ta), (float(np.median(tb)), tb)
    added = float(np.median(np.array(tb) - np.array(ta)))
    spread = float(max(np.ptp(ta), np.ptp(tb)))
    c = median_ms(scores, reps)
    eng.marginals()
    eng.sync()
    d = median_ms(host, reps)
    # the two routes agree (the device's rotation is of an unnormalised quaternion, numpy's of a normalised one: a few ulps)
    eng.marginals(pose=True)
    dev, ref = scores(), host_scores(eng, 0, n)
    agree = float(max(np.max(np.abs(dev[s] - ref[s]) / np.abs(ref[s]).max()) for s in dev))
    eng.close()
    resolved = added > spread            # else the extraction kernel is below what two timings of the whole call can tell apart
    res = dict(windows=windows, keyframes=n, marginals_ms=a, marginals_pose_ms=b, added_ms=added, call_spread_ms=spread, added_resolved=resolved,
               extraction_bytes=windows * n * BYTES_PER_KEYFRAME,
               hbm_fraction=windows * n * BYTES_PER_KEYFRAME / (added * 1e-3) / HBM_BYTES_PER_S if resolved else None,
               scores_and_read_ms=c, device_route_ms=(added if resolved else 0.0) + c[0],
               host_route_ms=d[0] * windows / hw, host_route_measured_ms=d, scaled_from=dict(windows_measured=hw, factor=windows / hw),
               routes_max_relative_difference=agree)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--host-windows", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_marginals_timing.json"))
    a = ap.parse_args()
    res = dict(one_window=measure(1, a.n, a.reps, a.host_windows), batch=measure(a.windows, a.n, a.reps, a.host_windows))
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
