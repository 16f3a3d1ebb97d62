"""How the View of one launch may differ from the engine's (vil_sensor_fusion_amd/csrc/vf_launch_view.hpp), against a table of every
variant and every composition the engine launches, byte by byte: tests/native/launch_view.cpp.  No GPU needed: the account is host
code, and the real vf_kernels.hpp compiles host-only against the HIP headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime.h")), reason="needs hip/hip_runtime.h")
def test_launch_view_table(tmp_path):
    exe = tmp_path / "launch_view"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE,
                           "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "launch_view.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "launch_view ok" in p.stdout
