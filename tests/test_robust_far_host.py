"""Robust losses on far between factors, what can be held without a GPU: the new entry points exist and validate their arguments
before they look at the engine, the handle's switch is a call that leaves vf_graph_opts alone, the Python layers carry the new arguments, and
robustify_between's stride is a compile-time parameter whose default is the band kernels' (their text names none)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np

from vil_sensor_fusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vf_engine_set_extra_between_robust", "vf_engine_get_extra_between_loss", "vf_engine_read_extra_lin", "vf_get_far_factors"]


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "vilfusion.h")).read()
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\b" + s + r"\(", hdr) and s in _lib.SYMBOLS and hasattr(l, s), s
    assert "int vf_set_robust_far(vf_graph* g, int on);" in hdr and "vf_set_robust_far" in _lib.SYMBOLS


def test_arguments_are_checked_before_the_engine():
    l = _lib.lib()
    a, b = np.array([1, 0, 3], dtype=np.int32), np.array([9, 6, 5], dtype=np.int32)
    rec = np.zeros((3, 28))
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))

    def call(loss, k):
        li, kk = np.array(loss, dtype=np.int32), np.array(k, dtype=np.float64)
        rc = l.vf_engine_set_extra_between_robust(None, 0, 3, ip(a), ip(b), dp(rec), ip(li), dp(kk))
        return rc, l.vf_last_error()
    for loss, k, what in (([1, 4, 0], [1.0, 1.0, 1.0], b"unknown loss id"), ([-1, 0, 0], [1.0, 1.0, 1.0], b"unknown loss id"),
                          ([1, 2, 0], [1.0, 0.0, 1.0], b"finite and > 0"), ([3, 0, 0], [math.inf, 1.0, 1.0], b"finite and > 0"),
                          ([0, 0, 2], [1.0, 1.0, math.nan], b"finite and > 0"), ([1, 2, 3], [1.0, 2.0, 3.0], b"engine is null"),
                          ([0, 0, 0], [-1.0, math.nan, 0.0], b"engine is null")):          # (k is ignored for VF_LOSS_NONE)
        rc, msg = call(loss, k)
        assert rc == -1 and what in msg, (loss, k, msg)
    assert l.vf_engine_set_extra_between_robust(None, 0, 3, ip(a), ip(b), dp(rec), None, None) == -1
    assert l.vf_engine_get_extra_between_loss(None, 0, None, None) == -1
    assert l.vf_engine_read_extra_lin(None, 0, 0, None, None, None) == -1
    assert l.vf_get_far_factors(None, None, None, None, None, None, None) == -1


def test_option_mirror_and_python_arguments():
    from vil_sensor_fusion_amd.engine import Engine
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    # the switch is a call on the handle, vf_set_robust_far: vf_graph_opts is the struct every caller built against it knows
    names = [f[0] for f in _lib.GraphOptsC._fields_]
    assert "robust_far" not in names and names[-1] == "far_covariance"
    assert _lib.lib().vf_set_robust_far(None, 1) == -1 and b"null" in _lib.lib().vf_last_error()
    assert inspect.signature(GraphManager.__init__).parameters["robust_far"].default is False
    p = inspect.signature(Engine.set_extra_between).parameters
    assert p["loss"].default is None and p["k"].default is None
    assert hasattr(Engine, "get_extra_between_loss") and hasattr(GraphManager, "far_weights")
    assert inspect.signature(Engine.read_extra_lin).parameters["which"].default == 0


def test_the_band_kernels_text_is_as_it_was():
    """robustify_between takes its stride as a template parameter that defaults to TILE; the band kernel calls it without one"""
    src = open(os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc", "kernels", "k12_linearize.inc")).read()
    assert "template <int STRIDE = TILE>\n__device__ __forceinline__ void robustify_between(" in src
    assert "if (RB && loss != LOSS_NONE) robustify_between(out, loss, loss_k);" in src
    far = open(os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc", "kernels", "far.inc")).read()
    assert "robustify_between<1>(out, fl.loss, fl.k)" in far and "template <bool RB>" in far
    lst = open(os.path.join(ROOT, "vil_sensor_fusion_amd", "csrc", "kernels.list")).read().split()
    assert "k_linearize_extra<false>" in lst and "k_linearize_extra<true>" in lst and "k_linearize_extra" not in lst
