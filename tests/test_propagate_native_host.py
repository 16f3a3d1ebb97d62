"""Host code of the IMU-rate prediction, as stand-alone programs built with -fsanitize=address,undefined and run as
programs: the step cut of vf_predict_state (vil_sensor_fusion_amd/csrc/vf_predict_steps.hpp, tests/native/predict_steps.cpp) and
the fact SolveMemory keeps about a propagation (vf_engine_memory.hpp, tests/native/engine_memory_propagate.cpp).  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", name + ".cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and name + " ok" in p.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_predict_steps(tmp_path):
    _build_and_run(tmp_path, "predict_steps")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_engine_memory_propagate(tmp_path):
    _build_and_run(tmp_path, "engine_memory_propagate")
