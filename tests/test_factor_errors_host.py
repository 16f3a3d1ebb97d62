"""Per-factor chi-square errors, the parts that need no GPU: when the engine may read the residuals a solve left as they lie
(SolveMemory::residuals_vouched, vil_sensor_fusion_amd/csrc/vf_engine_memory.hpp) against a table of event sequences,
tests/native/engine_memory_errors.cpp; the layout of the two output structs against their ctypes mirrors; the numpy reference of
the summaries (tests/errors_ref.py) on hand-made errors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import errors_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_residuals_fact_table(tmp_path):
    exe = tmp_path / "engine_memory_errors"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "engine_memory_errors.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and "engine_memory_errors ok" in p.stdout


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_output_structs_match_their_ctypes_mirrors(tmp_path):
    """vf_consistency and vf_batch_health as a C caller sees them (built the way tests/test_c_example.py builds its program: gcc,
    -std=c99, against include/vilfusion.h) against ConsistencyC and BatchHealthC: size, every offset, and no member the mirror lacks."""
    import re
    from vil_sensor_fusion_amd import _lib
    mirrors = {"vf_consistency": _lib.ConsistencyC, "vf_batch_health": _lib.BatchHealthC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', 'int main(void) {']
    for name, cls in mirrors.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines += ["return 0; }"]
    src = tmp_path / "errors_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "errors_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vilfusion.h")).read(), flags=re.S)
    for name, cls in mirrors.items():
        assert int(got[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f"{name}.{f}"
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", txt, flags=re.S).group(1)
        members = [m for decl in body.split(";") if decl.strip() for m in decl.split(",")]
        assert len(members) == len(cls._fields_), (name, len(members), len(cls._fields_))
        assert cls._fields_[0][0] == "struct_size" and getattr(cls, "struct_size").offset == 0
    assert (_lib.FACTOR_CLASSES, _lib.FACTOR_ROWS) == (("imu", "between", "prior", "marginal_prior", "far", "far_linear"), (15, 6, 15, 27, 6, 6))
    for i, name in enumerate(("IMU", "BETWEEN", "PRIOR", "MARGINAL_PRIOR", "FAR", "FAR_LINEAR")):
        assert re.search(rf"#define VF_FACTOR_{name} {i}\b", txt), name


def test_chi2_constants_and_thresholds():
    from vil_sensor_fusion_amd import CHI2_999, engine
    assert CHI2_999 == {6: 22.4577, 15: 37.6973, 27: 55.4760}
    assert list(engine._thresholds(CHI2_999)) == [37.6973, 22.4577, 37.6973, 55.4760, 22.4577, 22.4577]
    assert list(engine._thresholds({"between": 3.0})) == [0.0, 3.0, 0.0, 0.0, 0.0, 0.0]
    assert list(engine._thresholds(range(6))) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0] and engine._thresholds(None) is None


def test_reference_summary_on_hand_made_errors():
    """tests/errors_ref.py is what the GPU tests hold the device summaries to: its rules on a case small enough to check by eye"""
    imu = np.array([-1.0, 2.0, 0.5, np.nan, 2.0, -1.0])
    btw = np.array([-1.0, -1.0, 30.0, 1.0, -1.0, -1.0])
    far = np.array([4.0, -1.0])
    s = errors_ref.summary(imu, btw, k0=10, lo=10, hi=15, prior=(10, 0.25), marginal=None, far=far, far_linear=np.array([-1.0, -1.0]),
                           thresholds=[3.0, 22.4577, 0.1, np.nan, -5.0, np.inf])
    assert s["count"] == [4, 2, 1, 0, 1, 0]
    assert s["nonfinite"] == [1, 0, 0, 0, 0, 0]
    assert s["sum"] == [4.5, 31.0, 0.25, 0.0, 4.0, 0.0] and s["total"] == 4.5 + 31.0 + 0.25 + 0.0 + 4.0 + 0.0
    assert s["max"] == [2.0, 30.0, 0.25, -1.0, 4.0, -1.0]
    assert s["argmax"] == [11, 12, 10, -1, 0, -1]                  # the lowest slot of the tie at 2.0
    assert s["flagged"] == [2, 1, 1, 0, 0, 0]                      # thresholds that are not finite positive numbers flag nothing
    assert (s["keyframes"], s["rows"], s["unknowns"]) == (5, 4 * 15 + 2 * 6 + 15 + 6, 75)
    assert s["status"] == 1 | 2
    e = errors_ref.summary(np.zeros(0), np.zeros(0), k0=0, lo=0, hi=0, prior=None, marginal=None, far=far * 0 - 1, far_linear=far * 0 - 1, thresholds=None)
    assert e["count"] == [0] * 6 and e["total"] == 0.0 and e["status"] == 4 and e["rows"] == 0 and e["argmax"] == [-1] * 6
    h = errors_ref.health([s, e], costs=[1.0, 0.0], n_acc=[2, 0], n_fail=[0, 0])
    assert h == dict(windows=2, empty=1, failed=0, nonfinite=1, never_accepted=0, flagged_windows=1, worst_window=0,
                     worst_reduced_chi2=2.0 * s["total"] / 18)
