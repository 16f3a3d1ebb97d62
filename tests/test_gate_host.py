"""The innovation gate, the parts that need no GPU: what SolveMemory (vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) knows about a
gate result and about tail-only covariances, against a table of event sequences (tests/native/engine_memory_gate.cpp); the layout
of vf_gate_result against its ctypes mirror; SensorManager's use of the gate on a stand-in GraphManager."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gate_fact_table(tmp_path):
    exe = tmp_path / "engine_memory_gate"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "engine_memory_gate.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "engine_memory_gate ok" in p.stdout


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_gate_result_matches_its_ctypes_mirror(tmp_path):
    """vf_gate_result as a C caller sees it (gcc, -std=c99, against include/vilfusion.h) against GateResultC: size and every offset"""
    from vil_sensor_fusion_amd import _lib
    cls = _lib.GateResultC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(vf_gate_result));']
    for name, _ in cls._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(vf_gate_result, {name}));')
    lines += ['printf("theflags %u %u\\n", VF_GATE_FROM_ESTIMATE, VF_MARGINALS_TAIL);',
              'printf("thecodes %d %d %d %d %d\\n", VF_GATE_OK, VF_GATE_NONE, VF_GATE_OUT_OF_REACH, VF_GATE_DEGENERATE, VF_GATE_NO_COVARIANCE);',
              'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(re.match(r"(\w+) (.*)", l).groups() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == __import__("ctypes").sizeof(cls) == 208
    for name, _ in cls._fields_:
        assert int(out[name]) == getattr(cls, name).offset, name
    assert out["theflags"] == f"{_lib.GATE_FROM_ESTIMATE} {_lib.MARGINALS_TAIL}"
    assert out["thecodes"] == " ".join(str(s) for s in (_lib.GATE_OK, _lib.GATE_NONE, _lib.GATE_OUT_OF_REACH, _lib.GATE_DEGENERATE, _lib.GATE_NO_COVARIANCE))
    assert len(_lib.GATE_STATUS) == 5


class _Graph:
    """a GraphManager stand-in that records the calls and answers the gate from a script"""

    def __init__(self, answers):
        self.answers, self.calls, self.key = list(answers), [], 0

    def reserveNode(self, t):
        self.key += 1
        return self.key

    def gate_between(self, a, b, pose, cov, threshold):
        self.calls.append(("gate", a, b, threshold))
        r = self.answers.pop(0)
        if isinstance(r, Exception):
            raise r
        return r

    def addBetweenFactor(self, a, b, pose, cov):
        self.calls.append(("add", a, b))

    def solve(self):
        self.calls.append(("solve",))


def _feed(sm, n):
    from vil_sensor_fusion_amd.sensor_manager import Odometry
    out = []
    for k in range(n):
        sm.sensorCallback(0.05 * k)
        out.append(sm.odometryCallback(Odometry(0.05 * k, [0.1 * k, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])))
    return out


def test_sensor_manager_asks_the_gate_first():
    """with a threshold: a rejected increment is not added and is kept in `gated`, the keys advance as they always did; any other
    status, or a refusal, adds the factor as always and counts it in `ungated`.  Without one: not one call more than before."""
    from vil_sensor_fusion_amd._lib import VilFusionError
    from vil_sensor_fusion_amd.sensor_manager import SensorManager
    ok = dict(status="ok", rejected=False, nis=3.0)
    bad = dict(status="ok", rejected=True, nis=400.0)
    far = dict(status="out_of_reach", rejected=False, nis=float("nan"))
    g = _Graph([VilFusionError(-1, "no solve yet"), ok, bad, far, ok])
    sm = SensorManager(g, optimize_after_odom=True, max_time_skip=0.1, innovation_gate=22.46)
    out = _feed(sm, 7)
    assert out == [False, False, True, True, False, True, True]
    assert [c for c in g.calls if c[0] == "gate"] == [("gate", k, k + 1, 22.46) for k in range(1, 6)]
    assert [c for c in g.calls if c[0] == "add"] == [("add", 1, 2), ("add", 2, 3), ("add", 4, 5), ("add", 5, 6)]      # (3, 4) was rejected; (4, 5) starts at key 4
    assert len(sm.gated) == 1 and sm.gated[0][1] == (3, 4) and sm.gated[0][2] == 400.0 and np.isclose(sm.gated[0][0], 0.2)
    assert sm.ungated == 2 and sm.last_valid_key == 6
    assert sum(1 for c in g.calls if c[0] == "solve") == 4
    plain = _Graph([])
    out = _feed(SensorManager(plain, optimize_after_odom=True, max_time_skip=0.1), 7)
    assert out == [False, False] + [True] * 5 and all(c[0] != "gate" for c in plain.calls)
