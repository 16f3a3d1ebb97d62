#!/usr/bin/env python3
"""Generates tests/golden/degeneracy_axes_golden.npz by IMPORTING the reference's own Python
(degeneracy_detection_functions.py, and apply_degen_function / calc_roc of make_prettier_graphs.py)
with ROS modules stubbed, as make_degeneracy_golden.py does.  The inputs are the matrices and poses
of degeneracy_golden.npz, read back from that file.  Only inputs and outputs are stored; no
reference source travels.  Run here (not on the GPU box):

    python tests/golden/make_degeneracy_axes_golden.py

Contents:
  names                     the 25 functions: degen_funcs, condition_number, differential_entropy,
                            then jensen_bregman_0, kullback_leibler_0pose, kullback_leibler_0cov, condition_cov
  subsets                   all trans rot x y z roll pitch yaw
  {kind}_mats, {kind}_pose  kind in well / illcond / tunnel: the inputs of degeneracy_golden.npz
  {kind}_{subset}           (25, T) what apply_degen_function returns
  edge_mats, edge_pose      diagonal entries that are zero, negative and tiny (the 1x1 path)
  edge_{axis}               (25, T) for the six axes; NaN where the reference raised
  edge_raised               the functions that raised on some edge entry (no try in the reference)
  roc_is_degen, roc_score   a seeded label / score set; roc_tpr, roc_fpr what calc_roc returns
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

REF = "/root/reference/vil_fusion/python"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "degeneracy_axes_golden.npz")

for name in ("rospy", "vil_fusion", "vil_fusion.msg", "nav_msgs", "nav_msgs.msg", "rosbag", "tf",
             "tf.transformations", "matplotlib", "matplotlib.pyplot", "matplotlib.lines", "matplotlib.patches",
             "matplotlib.ticker", "matplotlib.font_manager", "matplotlib.axes"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["vil_fusion.msg"].DegeneracyScore = object
sys.modules["nav_msgs.msg"].Odometry = object


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


funcs = load(os.path.join(REF, "degeneracy_detection_functions.py"), "ref_degen_funcs")

# apply_degen_function and calc_roc are pure numpy; lift them out of make_prettier_graphs.py by executing their source
# text in an empty namespace (the module itself needs rosbag / matplotlib)
src = open(os.path.join(REF, "make_prettier_graphs.py")).read()
ns = {"np": np}
exec(compile(src[src.index("def apply_degen_function("):src.index("def plot_roc(")], "make_prettier_graphs", "exec"), ns)
apply_degen_function, calc_roc = ns["apply_degen_function"], ns["calc_roc"]

all_funcs = list(funcs.degen_funcs) + [funcs.condition_number, funcs.differential_entropy,
                                       funcs.jensen_bregman_0, funcs.kullback_leibler_0pose,
                                       funcs.kullback_leibler_0cov, funcs.condition_cov]
names = [f.__name__ for f in all_funcs]
SUBSETS = ["all", "trans", "rot", "x", "y", "z", "roll", "pitch", "yaw"]
AXES = SUBSETS[3:]

base = np.load(os.path.join(HERE, "degeneracy_golden.npz"))
out = {"names": np.array(names), "subsets": np.array(SUBSETS)}
warnings.simplefilter("ignore")
for kind in ("well", "illcond", "tunnel"):
    mats, pose = base[f"{kind}_mats"], base[f"{kind}_pose"]
    out[f"{kind}_mats"], out[f"{kind}_pose"] = mats, pose
    for subset in SUBSETS:
        out[f"{kind}_{subset}"] = np.stack([np.real(apply_degen_function(mats, pose, subset, f)) for f in all_funcs])

# the 1x1 path on entries that are zero, negative and tiny: each axis' diagonal runs through a sequence of such values
# (and ordinary ones between them), so every function meets them as the current and as the previous entry
rng = np.random.default_rng(20261015)
specials = np.array([0.0, -3.5, 1e-12, 2.0, 0.0, 0.0, -1e-12, 7.25, -0.5, -0.5, 1e-30, 4e3, 0.0, 1.0, -2e-9, 3.0])
T = 48
edge = np.zeros((6, 6, T))
for a in range(6):
    seq = np.roll(np.concatenate([specials, rng.uniform(0.1, 100.0, T - len(specials))]), 5 * a)
    edge[a, a, :] = seq
    for b in range(6):
        if b != a:
            edge[a, b, :] = rng.normal(size=T) * 0.1       # the off-diagonal entries never reach a 1x1
edge_pose = rng.normal(size=(6, 1, T))
out["edge_mats"], out["edge_pose"] = edge, edge_pose
raised = set()


def guarded(f):
    """f, with the reference's uncaught LinAlgError (norm_*_ratio of a singular previous entry) recorded as NaN"""
    def g(**kw):
        try:
            return f(**kw)
        except np.linalg.LinAlgError:
            raised.add(f.__name__)
            return np.nan
    return g


for axis in AXES:
    out[f"edge_{axis}"] = np.stack([np.real(apply_degen_function(edge, edge_pose, axis, guarded(f))) for f in all_funcs])
out["edge_raised"] = np.array(sorted(raised))

# calc_roc on a seeded score / label set (ties included: the scores are rounded)
score = np.round(rng.normal(size=400), 2)
is_degen = rng.uniform(size=400) < 1.0 / (1.0 + np.exp(3.0 * score))
tpr, fpr = calc_roc(is_degen, score)
out.update(roc_is_degen=is_degen, roc_score=score, roc_tpr=tpr, roc_fpr=fpr)

np.savez_compressed(OUT, **out)
print("wrote", OUT, {k: v.shape for k, v in out.items() if k not in ("names", "subsets")})
print("raised:", sorted(raised))
