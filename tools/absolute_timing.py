"""K2 with and without absolute factors at the headline shape (1 024 windows x 1 000 keyframes): vf_engine_time_stage(VF_STAGE_LINEARIZE_BTW)
and the time of a 5-trial step, every figure the median of 9, per library, each library in a child process of its own and the two
libraries alternating (boxes differ by +-5 %, K4 by +-3-4 % between processes: README; NOTEBOOK 7.18 alternates the same way).
usage: python tools/absolute_timing.py <parent's libvilfusion.so> [<this tree's .so>] [--pairs P] [--out profiles/absolute_timing.json]
A library without vf_engine_set_absolute (the parent commit's) is measured with no absolute factor only.  The one claim the record is
for: this library with no absolute factor lies within the parent's own run-to-run spread of the same run ("within_parent_spread")."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def driver(argv):
    pairs, out = 3, None
    libs = [a for a in argv if a.endswith(".so")]
    if "--pairs" in argv:
        pairs = int(argv[argv.index("--pairs") + 1])
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if len(libs) == 1:
        libs.append(os.path.join(ROOT, "vil_sensor_fusion_amd", "libvilfusion.so"))
    runs = []
    for _ in range(pairs):
        for role, so in zip(("parent", "tree"), libs):
            line = subprocess.run([sys.executable, __file__, "--child", os.path.abspath(so)], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
            runs.append(dict(role=role, **json.loads(line)))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for key in ("k2_ms", "step5_ms"):
        par = [r["none"][key] for r in runs if r["role"] == "parent"]
        tree = [r["none"][key] for r in runs if r["role"] == "tree"]
        summary[key] = dict(parent=par, tree_no_absolute_factor=tree, parent_spread=max(par) - min(par),
                            within_parent_spread=bool(min(par) <= statistics.median(tree) <= max(par)))
    rec = dict(windows=1024, keyframes=1000, median_of=9, pairs=pairs, summary=summary, runs=runs)
    print(json.dumps(rec["summary"]))
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


def child(so):
    sys.path.insert(0, ROOT)
    import numpy as np
    from vil_sensor_fusion_amd import _lib
    _lib._SO = so
    from vil_sensor_fusion_amd import Engine, EngineOpts, synth
    from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS

    B, N = 1024, 1000
    seq = synth.make_sequence(0, N)
    eng = Engine(EngineOpts(windows=B, capacity=N))
    rec = synth.between_records(seq)

    def load_between():
        for w in range(B):
            eng.set_between(w, seq.btw_a, seq.btw_b, rec)

    for w in range(B):
        eng.preintegrate(w, 1, seq.imu_off[1:], seq.imu_steps, np.zeros(6), synth.CARLA_IMU_COV)
        eng.set_states(w, 0, seq.gt_states[:1])
        eng.set_prior(w, 0, synth.prior_record(seq.gt_states[0], REFERENCE_PRIOR_SIGMAS))
        eng.set_range(w, 0, 1)
        eng.predict(w, 1, N - 1)
        eng.set_range(w, 0, N)
    load_between()
    start = [eng.get_states(w, 0, N) for w in (0,)][0]

    def measure():
        for w in range(B):                          # (every configuration from the same states)
            eng.set_states(w, 0, start)
        eng.linearize(0)
        eng.decide(init=True)
        eng.sync()
        k2 = [eng.time_stage("linearize_between", 20) for _ in range(9)]
        it = [eng.time_iterate(5) for _ in range(9)]
        return dict(k2_ms=round(statistics.median(k2), 4), step5_ms=round(statistics.median(it), 3),
                    k2_spread=round(max(k2) - min(k2), 4), step5_spread=round(max(it) - min(it), 3))

    out = dict(library=os.path.basename(os.path.dirname(so)) + "/" + os.path.basename(so), none=measure())
    if hasattr(eng._l, "vf_engine_set_absolute"):
        iso = np.zeros(28)
        iso[7 + np.array([0, 6, 11, 15, 18, 20])] = 1.0 / 0.05

        def fixes(slots, kinds):
            """ground-truth fixes with an isotropic 0.05 square-root covariance: a pose's record, or a position's (translation block only)"""
            r = np.zeros((len(slots), 28))
            for i, (k, kind) in enumerate(zip(slots, kinds)):
                r[i] = iso
                if kind == _lib.ABSOLUTE_POSITION:
                    r[i, 7:7 + 15] = 0.0
                    r[i, 0] = 1.0
                else:
                    r[i, 0:4] = seq.gt_states[k, 0:4]
                r[i, 4:7] = seq.gt_states[k, 4:7]
            return r
        # the array present and empty: a factor on the slot behind nothing, cleared again
        eng.set_absolute(0, [1], "pose", fixes([1], [_lib.ABSOLUTE_POSE]))
        eng.clear_between(0, 1, 1)
        load_between()
        assert not eng.get_absolute(0, 0, N).any()
        out["array_empty"] = measure()
        tenth = list(range(10, N, 10))
        for w in range(B):
            eng.set_absolute(w, tenth, "pose", fixes(tenth, [_lib.ABSOLUTE_POSE] * len(tenth)))
        out["one_slot_in_ten_a_pose_fix"] = dict(measure(), fixes=len(tenth))
        load_between()
        free = sorted(set(range(1, N)) - set(int(b) for b in seq.btw_b))
        kinds = [_lib.ABSOLUTE_POSE if i % 2 else _lib.ABSOLUTE_POSITION for i in range(len(free))]
        for w in range(B):
            eng.set_absolute(w, free, kinds, fixes(free, kinds))
        out["every_free_slot_a_fix"] = dict(measure(), fixes=len(free))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) >= 2 and any(a.endswith(".so") for a in sys.argv[1:]):
        driver(sys.argv[1:])
    else:
        sys.exit(__doc__)
