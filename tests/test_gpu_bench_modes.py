"""-m gpu: the two ways bench.py runs.  A plain run measures the headline figure and nothing else; --full adds every other
section.  Both must time the same engine on the same inputs, so what --dump-outputs writes is the same, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sections of a --full line and report that a plain run must not have paid for
FULL_ONLY = ("accuracy", "stage_ms", "roofline", "roofline_solve", "solve_form", "cpu_baseline", "cpu_baseline_all_cores",
             "with_convergence_exit", "incremental_update", "single_window", "graph_manager", "time_sharded_window",
             "degeneracy_k6", "degeneracy_k6_ns_per_matrix", "profiled_kernels")
# a small batch; the switches keep the --full run to the sections that size the engine and the sequences (the accuracy
# reference and the convergence-exit updates) plus the per-kernel figures, the others are covered where they are tested
SHAPE = ["--gpus", "1", "--windows", "8", "--window", "96", "--steps", "2", "--warmup", "1", "--init-iterations", "30",
         "--cpu-steps", "4", "--accuracy-windows", "1", "--host-workers", "1",
         "--no-sharded", "--no-degeneracy", "--no-graph-manager", "--no-single-window", "--no-incremental"]


def _start(tmp_path, name, extra):
    out = tmp_path / name
    out.mkdir()
    env = dict(os.environ, VF_BENCH_DETAIL_DIR=str(out))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + SHAPE + extra + ["--dump-outputs", str(out / "dump")]
    return out, subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(proc):
    stdout, stderr = proc.communicate(timeout=600)
    assert proc.returncode == 0, stderr[-2000:]
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_full_run_times_the_same_thing(tmp_path):
    plain_dir, plain = _start(tmp_path, "plain", [])
    full_dir, full = _start(tmp_path, "full", ["--full"])
    plain, full = _finish(plain), _finish(full)
    for line in (plain, full):
        assert line["metric"].startswith("keyframes/sec") and line["unit"] == "keyframes/s" and line["dtype"] == "f64"
        assert line["higher_is_better"] is True and line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and abs(line["value"] / (8 / (line["ms_per_step"] * 1e-3)) - 1) < 1e-4
    assert plain["config"] == full["config"]
    plain_detail = json.load(open(plain_dir / "bench_detail.json"))
    for k in FULL_ONLY:
        assert k not in plain, k
        assert plain_detail.get(k) is None, k
    for k in ("accuracy", "stage_ms", "roofline", "roofline_solve", "with_convergence_exit"):
        assert k in full, k
    assert "cpu_baseline" in json.load(open(full_dir / "bench_detail.json"))
    # same inputs, same engine, same steps: the outputs of the last timed step agree bit for bit
    for name in ("lm", "states_windows", "states"):
        a, b = np.load(plain_dir / "dump" / f"{name}.npy"), np.load(full_dir / "dump" / f"{name}.npy")
        assert a.shape == b.shape and a.size > 0
        np.testing.assert_array_equal(a, b)
