"""The engine's upload channel and the owner of its events (vil_sensor_fusion_amd/csrc/vf_upload_channel.hpp, vf_device_buf.hpp)
against logging stubs of the HIP calls they make: tests/native/upload_channel.cpp, a program of its own, built plainly and with
AddressSanitizer + UBSan.  No GPU needed, and no HIP runtime: only its headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_upload_channel_table(tmp_path, sanitize):
    exe = tmp_path / "upload_channel"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                           "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"), *sanitize,
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "upload_channel.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "upload_channel ok" in p.stdout
