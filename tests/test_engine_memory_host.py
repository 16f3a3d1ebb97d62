"""What the engine remembers from one solve to the next and which call voids it (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp),
against a table of event sequences: tests/native/engine_memory.cpp.  No GPU needed: the account is host code, and every entry
point of the engine reports to it and asks it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_engine_memory_table(tmp_path):
    exe = tmp_path / "engine_memory"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "engine_memory.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "engine_memory ok" in p.stdout
