"""Pose marginals in nav_msgs layout and their degeneracy scores, host side (no device): the five new entry points are exported and
declared, their flag and source constants are those of the header, NULL handles are refused, and the Python arguments exist."""
import ctypes as C
import inspect
import os
import subprocess

from vil_sensor_fusion_amd import _lib

NEW = ["vf_engine_read_pose_marginals", "vf_engine_marginal_scores", "vf_engine_read_marginal_scores", "vf_get_degeneracy_scores"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported():
    import __graft_entry__ as g
    if not os.path.exists(_lib.lib_path()):
        g.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW + ["vf_engine_marginals_ex"]:
        assert s in have and s in _lib.SYMBOLS, s
    hdr = open(os.path.join(ROOT, "include", "vilfusion.h")).read()
    assert "#define VF_MARGINALS_POSE 2u" in hdr and _lib.MARGINALS_POSE == 2
    assert "#define VF_SCORE_COVARIANCE 0" in hdr and "#define VF_SCORE_INFORMATION 1" in hdr
    assert (_lib.SCORE_COVARIANCE, _lib.SCORE_INFORMATION) == (0, 1)


def test_null_handles_are_refused():
    l = _lib.lib()
    buf = (C.c_double * 36)()
    assert l.vf_engine_marginals_ex(None, _lib.MARGINALS_POSE) == -1
    assert l.vf_engine_marginals_ex(None, _lib.MARGINALS_POSE | _lib.MARGINALS_FAR) == -1
    assert l.vf_engine_read_pose_marginals(None, 0, 0, 1, buf, None, None) == -1
    assert b"null" in l.vf_last_error()
    assert l.vf_engine_marginal_scores(None, 0, 0, 7) == -1
    assert b"null" in l.vf_last_error()
    assert l.vf_engine_read_marginal_scores(None, 0, 0, 1, buf) == -1
    assert b"null" in l.vf_last_error()
    assert l.vf_get_degeneracy_scores(None, 0, 0, 7, 0, 1, buf) == -1
    assert b"null" in l.vf_last_error()


def test_the_handle_entry_lives_outside_vf_graph_cpp():
    """the host tests link vf_graph.cpp against a stand-in engine without the new engine calls: it must not name them"""
    csrc = os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc")
    g = open(os.path.join(csrc, "vf_graph.cpp")).read()
    for s in NEW:
        assert s not in g, s
    assert '#include "vf_graph_handle.hpp"' in g
    assert "vf_get_degeneracy_scores" in open(os.path.join(csrc, "vf_graph_scores.cpp")).read()
    assert "vf_graph_scores.o" in open(os.path.join(csrc, "Makefile")).read()


def test_python_arguments():
    from vil_sensor_fusion_amd.engine import Engine
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    p = inspect.signature(Engine.marginals).parameters
    assert p["far"].default is False and p["pose"].default is False
    assert inspect.signature(Engine.marginal_scores).parameters["information"].default is False
    assert hasattr(Engine, "read_pose_marginals") and hasattr(Engine, "read_marginal_scores")
    p = inspect.signature(GraphManager.degeneracy_scores).parameters
    assert p["information"].default is False and p["key0"].default is None and p["n"].default is None
