"""K2 with and without robust losses at the headline shape (1 024 windows x 1 000 keyframes): vf_engine_time_stage(VF_STAGE_LINEARIZE_BTW)
and the time of a 5-trial solve, per library variant, each variant in a child process of its own (boxes differ by +-5 %, K4 by
+-3-4 % between processes: README).
usage: python tools/robust_timing.py <variant.so> ...   one JSON line per run; a library without vf_engine_set_between_loss
       (the parent commit's) is measured with the loss off only.  profiles/robust_timing.json is a run of this tool."""
import json
import os
import subprocess
import sys

if len(sys.argv) > 2 or (len(sys.argv) == 2 and not sys.argv[1].endswith(".so")):
    for so in sys.argv[1:]:
        subprocess.run([sys.executable, __file__, os.path.abspath(so)], check=True)
    sys.exit(0)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from vil_sensor_fusion_amd import _lib  # noqa: E402
_lib._SO = sys.argv[1]
from vil_sensor_fusion_amd import Engine, EngineOpts, synth  # noqa: E402
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS  # noqa: E402

B, N = 1024, 1000
seq = synth.make_sequence(0, N)
eng = Engine(EngineOpts(windows=B, capacity=N))
rec = synth.between_records(seq)
for w in range(B):
    eng.preintegrate(w, 1, seq.imu_off[1:], seq.imu_steps, np.zeros(6), synth.CARLA_IMU_COV)
    eng.set_between(w, seq.btw_a, seq.btw_b, rec)
    eng.set_states(w, 0, seq.gt_states[:1])
    eng.set_prior(w, 0, synth.prior_record(seq.gt_states[0], REFERENCE_PRIOR_SIGMAS))
    eng.set_range(w, 0, 1)
    eng.predict(w, 1, N - 1)
    eng.set_range(w, 0, N)


def measure():
    eng.linearize(0)
    eng.decide(init=True)
    eng.sync()
    k2 = [eng.time_stage("linearize_between", 20) for _ in range(5)]
    k1 = [eng.time_stage("linearize_imu", 10) for _ in range(3)]
    it = [eng.time_iterate(5) for _ in range(3)]
    return dict(k2_ms=[round(x, 4) for x in k2], k1_ms=[round(x, 4) for x in k1], iterate5_ms=[round(x, 3) for x in it])


out = dict(library=os.path.basename(sys.argv[1]), windows=B, keyframes=N, loss_off=measure())
if hasattr(eng._l, "vf_engine_set_between_loss"):
    for w in range(B):
        eng.set_between_loss(w, seq.btw_b, "huber", 1.345)
    out["huber_on_every_factor"] = measure()
    # (on the synthetic data every factor is an inlier at 1.345: the pass reads r and returns.  A threshold every factor is beyond:)
    for w in range(B):
        eng.set_between_loss(w, seq.btw_b, "huber", 1e-6)
    out["huber_every_factor_an_outlier"] = measure()
print(json.dumps(out), flush=True)
