"""The loop-closure gate, the parts that need no GPU: what SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) knows about
its records, against a table of event sequences (tests/native/engine_memory_closure.cpp); the layout of vf_closure_gate_result
against its ctypes mirror."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_closure_fact_table(tmp_path):
    exe = tmp_path / "engine_memory_closure"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "engine_memory_closure.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "engine_memory_closure ok" in p.stdout


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_closure_gate_result_matches_its_ctypes_mirror(tmp_path):
    """vf_closure_gate_result as a C caller sees it (gcc, -std=c99, against include/vilfusion.h) against ClosureGateResultC: size and
    every offset; VF_CLOSURE_GATE_MAX against its Python twin"""
    from vil_sensor_fusion_amd import _lib
    cls = _lib.ClosureGateResultC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(vf_closure_gate_result));']
    for name, _ in cls._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(vf_closure_gate_result, {name}));')
    lines += ['printf("themax %d\\n", VF_CLOSURE_GATE_MAX);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(re.match(r"(\w+) (.*)", l).groups() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 88
    for name, _ in cls._fields_:
        assert int(out[name]) == getattr(cls, name).offset, name
    assert int(out["themax"]) == _lib.CLOSURE_GATE_MAX == 4
