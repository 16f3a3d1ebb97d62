"""What a robust loss on loop closures costs a vf_solve: a GraphManager at a 1 000-keyframe lag, one keyframe per solve, with one and
with eight closures alive -- loss off, Huber with every closure an inlier, Huber with every closure an outlier -- per library
variant, each run in a child process of its own.

usage: python tools/robust_far_timing.py <variant.so> ...   one JSON line per (library, mode); a library without
       vf_engine_set_extra_between_robust (the parent commit's) is measured with the loss off only.
       profiles/robust_far_timing.json holds runs of this tool, parent and this commit alternating on one box."""
import json
import os
import subprocess
import sys
import time

MODES = {"off": None, "huber_all_inliers": ("huber", 1e6), "huber_all_outliers": ("huber", 1e-9)}

if len(sys.argv) < 3 or sys.argv[2] not in MODES:
    for so in sys.argv[1:]:
        for mode in MODES:
            subprocess.run([sys.executable, __file__, os.path.abspath(so), mode], check=True)
    sys.exit(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes  # noqa: E402
import numpy as np  # noqa: E402
from vil_sensor_fusion_amd import _lib  # noqa: E402
_lib._SO = sys.argv[1]
if MODES[sys.argv[2]] is not None and not hasattr(ctypes.CDLL(sys.argv[1]), "vf_engine_set_extra_between_robust"):
    sys.exit(0)
from tests.test_gpu_far_factors import _far_record          # noqa: E402
from tests.test_gpu_graph_manager import _stream            # noqa: E402
from vil_sensor_fusion_amd import synth                     # noqa: E402
from vil_sensor_fusion_amd.graph_manager import GraphManager  # noqa: E402

robust = MODES[sys.argv[2]]
WARM, MEASURE = 1010, 30
n = WARM + 2 * (MEASURE + 10) + 10
seq = synth.make_sequence(7, n)
traj_t, acc, gyr = _stream(seq)
rng = np.random.default_rng(3)
gm = GraphManager(capacity=2048, lag=1000, iterations=5, max_far_factors=32, robust_far=robust is not None)
gm.setInitialState(seq.gt_states[0])
i_imu, alive, rows = 0, 0, {1: [], 8: []}
for k in range(1, n):
    while i_imu < traj_t.size and traj_t[i_imu] <= seq.kf_time[k] + 0.01:
        gm.addIMUMeasurement(traj_t[i_imu], acc[i_imu], gyr[i_imu])
        i_imu += 1
    gm.reserveNode(seq.kf_time[k])
    for a, b, q, t, c in zip(seq.btw_a, seq.btw_b, seq.btw_q, seq.btw_t, seq.btw_cov):
        if b == k and a >= 1:
            gm.addBetweenFactor(int(a), int(b), (q, t), np.eye(6) * c)
    new = 0
    want = 1 if k == WARM else 8 if k == WARM + MEASURE + 10 else alive          # one closure, then eight at once
    while alive < want:
        a = k - int(rng.integers(200, 900))
        rec = _far_record(seq, a, k, rng, cov=1e-2, noise=(1e-3, 1e-2))
        gm.addBetweenFactor(a, k, (rec[0:4], rec[4:7]), np.eye(6) * 1e-2, robust=robust)
        alive += 1
        new += 1
    t0 = time.perf_counter()
    gm.solve()
    dt = (time.perf_counter() - t0) * 1e3
    if not new and alive in rows and len(rows[alive]) < MEASURE + 5:
        rows[alive].append(dt)
st = gm.lmStats()
weights = [round(w, 6) for *_, w in gm.far_weights()] if hasattr(gm._l, "vf_get_far_factors") else None
gm.close()
out = dict(library=os.path.basename(os.path.dirname(sys.argv[1])) + "/" + os.path.basename(sys.argv[1]), mode=sys.argv[2], lag=1000, trials_at_most=5)
for c, v in rows.items():
    v = np.array(v[5:])          # (the first solves behind a new closure run more trials)
    out[f"vf_solve_ms_{c}_closures"] = dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4), solves=int(v.size))
out["solve_failures"] = st["solve_failures"]
out["closure_weights_at_the_end"] = weights
print(json.dumps(out), flush=True)
