"""Which of its two kernels the back substitution of a split or assembling sweep takes (vf_solve_plan.hpp, backsub_one_wave;
vf_engine_tuning.solve_backsub_form): batches of SIMD count - 1, SIMD count and SIMD count + 1, the forcing field, the plans that
have no such kernel -- and every plan of tests/native/solve_plan.cpp's table as it was while the two new inputs keep their
defaults.  tests/native/solve_plan_backsub.cpp; host code, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_backsub_form_rule(tmp_path):
    exe = tmp_path / "solve_plan_backsub"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "solve_plan_backsub.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "solve_plan ok" in p.stdout and "solve_plan backsub ok" in p.stdout
