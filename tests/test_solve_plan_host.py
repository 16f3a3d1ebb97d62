"""The policy that picks the band solve's form, what K3 does around it and the factor kernel of the marginal covariances
(vil_sensor_fusion_amd/csrc/vf_solve_plan.hpp), against a table of batches, tunings and engine states: tests/native/solve_plan.cpp.
No GPU needed: the plan is host code, and every launcher and entry point takes its decisions from it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_solve_plan_table(tmp_path):
    exe = tmp_path / "solve_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "solve_plan.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "solve_plan ok" in p.stdout
