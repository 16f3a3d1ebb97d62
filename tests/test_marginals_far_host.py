"""Marginal covariances with far factors alive, host side (no device): the new entry point and flag, the handle option's ctypes
mirror and default, and the Python arguments."""
import ctypes as C
import inspect
import os
import subprocess

from vil_sensor_fusion_amd import _lib


def test_new_symbol_is_exported():
    import __graft_entry__ as g
    if not os.path.exists(_lib.lib_path()):
        g.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "vf_engine_marginals_ex" in have and "vf_engine_marginals_ex" in _lib.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vilfusion.h")).read()
    assert "#define VF_MARGINALS_FAR 1u" in hdr and _lib.MARGINALS_FAR == 1


def test_null_engine_is_refused_with_and_without_the_flag():
    l = _lib.lib()
    assert l.vf_engine_marginals_ex(None, _lib.MARGINALS_FAR) == -1
    assert l.vf_engine_marginals_ex(None, 0) == -1
    assert b"null" in l.vf_last_error()


def test_graph_option_mirror_and_default():
    names = [f[0] for f in _lib.GraphOptsC._fields_]
    assert names[-1] == "far_covariance"
    o = _lib.GraphOptsC()
    _lib.lib().vf_graph_default_opts_sized(C.byref(o), C.sizeof(o))
    assert o.struct_size == C.sizeof(o) and o.far_covariance == 0


def test_python_arguments():
    from vil_sensor_fusion_amd.engine import Engine
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    assert inspect.signature(Engine.marginals).parameters["far"].default is False
    assert inspect.signature(GraphManager.__init__).parameters["far_covariance"].default is False
