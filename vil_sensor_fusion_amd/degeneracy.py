"""Batched degeneracy metrics on the GPU (K6): the counterpart of the reference's
apply_degen_function (vil_fusion/python/make_prettier_graphs.py:547-576), its ROC helper calc_roc
(:579-588), and the shipped D-optimality gate (gtsam_fusion/src/degerate_odometry_filter.cpp:29-47)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

# order of degen_funcs (vil_fusion/python/degeneracy_detection_functions.py:283-303) + 2 extras
METRICS = ["d_opt", "d_opt_ratio", "a_opt", "a_opt_ratio", "e_opt", "e_opt_ratio", "max_eigen",
           "max_eigen_ratio", "jensen_bregman", "correlation_matrix_distance", "kullback_leibler",
           "norm_frobenius", "norm_frobenius_ratio", "norm_nuclear", "norm_nuclear_ratio", "norm_1",
           "norm_1_ratio", "norm_2", "norm_2_ratio", "condition_number", "differential_entropy"]
# the variants of degeneracy_detection_functions.py:184-193, 247-251 (metric ids 21 .. 24, after METRICS)
EXTRA_METRICS = ["jensen_bregman_0", "kullback_leibler_0pose", "kullback_leibler_0cov", "condition_cov"]
# subset ids of include/vilfusion.h (VF_SUBSET_*): the 6x6, its two 3x3 blocks, the 1x1 entry of each axis
SUBSETS = {"all": 0, "trans": 1, "rot": 2, "x": 3, "y": 4, "z": 5, "roll": 6, "pitch": 7, "yaw": 8}
ALL_METRICS = METRICS + EXTRA_METRICS
ROT_DEGEN_THRESHOLD, TRANS_DEGEN_THRESHOLD = 11.5, 28.9     # config/carla/fusion_params.yaml:35-36


def _metric_id(func):
    name = func if isinstance(func, str) else func.__name__
    if name not in ALL_METRICS:
        raise KeyError(f"metric {name!r} is not implemented on the GPU")
    return ALL_METRICS.index(name)


def _stage(matrix, pose, dtype):
    m = np.ascontiguousarray(np.asarray(matrix).transpose(2, 0, 1), dtype=dtype)
    if m.shape[1:] != (6, 6):
        raise ValueError("matrix must be (6,6,T)")
    p = None
    if pose is not None:
        p = np.ascontiguousarray(np.asarray(pose)[:, 0, :].T, dtype=dtype)
    return m, p


def apply_degen_function(matrix, pose, matrix_subset, func, dtype=np.float64, reps=0):
    """Same contract as the reference: matrix (6,6,T), pose (6,1,T) or None, subset in
    {"all","trans","rot","x","y","z","roll","pitch","yaw"}, func = metric name (or a reference
    function object, matched by __name__).  Returns y (T,), y[0] = 0.  With reps > 0 also returns
    the kernel time in ms."""
    metric = _metric_id(func)
    if matrix_subset not in SUBSETS:
        raise RuntimeWarning("Invalid matrix subset {}".format(matrix_subset))   # as the reference (:560)
    m, p = _stage(matrix, pose, dtype)
    out = np.zeros(m.shape[0], dtype=dtype)
    ms = C.c_float(0)
    check(_lib.lib().vf_degeneracy_batch(
        m.ctypes.data_as(C.c_void_p), None if p is None else p.ctypes.data_as(C.c_void_p), m.shape[0],
        0 if dtype == np.float64 else 1, SUBSETS[matrix_subset], metric,
        out.ctypes.data_as(C.c_void_p), reps, C.byref(ms)))
    return (out, ms.value) if reps > 0 else out


def scores(matrix, pose, func, subsets=("all", "trans", "rot"), dtype=np.float64, reps=0):
    """One metric on several subsets of every matrix of a (6,6,T) stack in ONE launch (each matrix read once): the
    online node's score_all / score_trans / score_rot by default (vil_fusion/src/vil_fusion/degeneracy_detection.py:115-130).
    Returns {subset: y (T,)}, each bit for bit what apply_degen_function returns for that subset (and the kernel time
    in ms with reps > 0)."""
    metric = _metric_id(func)
    for s in subsets:
        if s not in SUBSETS:
            raise RuntimeWarning("Invalid matrix subset {}".format(s))
    rows = sorted({SUBSETS[s] for s in subsets})
    mask = sum(1 << r for r in rows)
    m, p = _stage(matrix, pose, dtype)
    out = np.zeros((len(rows), m.shape[0]), dtype=dtype)
    ms = C.c_float(0)
    check(_lib.lib().vf_degeneracy_scores_batch(
        m.ctypes.data_as(C.c_void_p), None if p is None else p.ctypes.data_as(C.c_void_p), m.shape[0],
        0 if dtype == np.float64 else 1, metric, C.c_uint(mask), out.ctypes.data_as(C.c_void_p), reps, C.byref(ms)))
    res = {s: out[rows.index(SUBSETS[s])] for s in subsets}
    return (res, ms.value) if reps > 0 else res


def calc_roc(is_degen, score):
    """ROC of a degeneracy score (make_prettier_graphs.py:579-588): a message counts as flagged at threshold t when its
    score is <= t, for the 100 thresholds at the 0th .. 100th percentile of the scores.  Returns (tpr, fpr), each (100,)."""
    score = np.asarray(score)
    truth = np.asarray(is_degen, dtype=bool)
    thresholds = np.percentile(score, np.linspace(0.0, 100.0, 100))
    flagged = score[None, :] <= thresholds[:, None]
    tpr = (flagged & truth).sum(axis=1) / truth.sum()
    fpr = (flagged & ~truth).sum(axis=1) / (~truth).sum()
    return tpr, fpr


def spectrum(matrix, matrix_subset="all", dtype=np.float64, reps=0):
    """e_opt, max_eigen and condition_number of every matrix of a (6,6,T) stack from ONE eigen-solve each (one launch, three
    outputs; bit for bit what three apply_degen_function calls return).  condition_number is NaN where a matrix is not
    symmetric to rounding.  Returns a dict (and the kernel time in ms with reps > 0)."""
    if matrix_subset not in SUBSETS:
        raise RuntimeWarning("Invalid matrix subset {}".format(matrix_subset))
    m, _ = _stage(matrix, None, dtype)
    outs = [np.zeros(m.shape[0], dtype=dtype) for _ in range(3)]
    ms = C.c_float(0)
    check(_lib.lib().vf_degeneracy_spectrum_batch(m.ctypes.data_as(C.c_void_p), m.shape[0], 0 if dtype == np.float64 else 1, SUBSETS[matrix_subset],
                                                 *[o.ctypes.data_as(C.c_void_p) for o in outs], reps, C.byref(ms)))
    res = dict(e_opt=outs[0], max_eigen=outs[1], condition_number=outs[2])
    return (res, ms.value) if reps > 0 else res


def eigen_threshold(log_det_threshold):
    """the eigenvalue at which a 3x3 block with three equal eigenvalues has exactly the log det the shipped gate tests"""
    return float(np.exp(float(log_det_threshold) / 3.0))


REMAP_ORDERS = {"loam": 0, "pose3": 1}      # out_order of vf_degeneracy_remap_batch: [trans, rot] as the input / [rot, trans]
POSE3_FROM_LOAM = np.array([3, 4, 5, 0, 1, 2])     # the block permutation between the two (its own inverse)


def remap_covariance(hessians, nom6, trans_thr=eigen_threshold(TRANS_DEGEN_THRESHOLD), rot_thr=eigen_threshold(ROT_DEGEN_THRESHOLD),
                     floor=1e-6, order="loam", dtype=np.float64, reps=0):
    """Deweight what a scan did not observe (vf_degeneracy_remap_batch; no reference code): (n,36) or (n,6,6) scan-matching
    Hessians in LOAM order [trans 3, rot 3] and the nominal covariance nom6 of the six axes in that order -> (cov (n,6,6),
    sqrt_info (n,21), eig (n,6), deweighted (n,)).  An eigen-direction of the threshold-scaled Hessian whose eigenvalue l' is
    below 1 keeps the share clamp(l', floor, 1) of its nominal information; the others keep all of it, and where deweighted is
    0 cov is diag(nom6) to the bit.  sqrt_info is the upper triangle of R = chol(cov^-1) by rows (words 7 .. 27 of a between
    record), eig the eigenvalues of the symmetrised Hessian itself, ascending.  order="pose3": cov and sqrt_info in the
    factor's tangent order [rot, trans].  dtype: what the Hessians are handed over as (float32 is promoted on the device; all
    outputs are float64).  A non-finite Hessian gives deweighted -1, cov = diag(nom6) / floor and NaN eigenvalues.  With
    reps > 0 also returns the kernel time in ms."""
    if order not in REMAP_ORDERS:
        raise ValueError(f"order must be one of {sorted(REMAP_ORDERS)}")
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    h =np.ascontiguousarray(hessians, dtype=dtype).reshape(-1, 36)
    nom = np.ascontiguousarray(nom6, dtype=np.float64).reshape(-1)
    if nom.size != 6:
        raise ValueError("nom6 must hold six values")
    n = h.shape[0]
    cov, sq, eig, dw = np.zeros((n, 6, 6)), np.zeros((n, 21)), np.zeros((n, 6)), np.zeros(n, np.int32)
    ms = C.c_float(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(_lib.lib().vf_degeneracy_remap_batch(vp(h), n, 0 if np.dtype(dtype) == np.float64 else 1, vp(nom), float(trans_thr), float(rot_thr),
                                               float(floor), REMAP_ORDERS[order], vp(cov), vp(sq), vp(eig), vp(dw), reps, C.byref(ms)))
    return (cov, sq, eig, dw, ms.value) if reps > 0 else (cov, sq, eig, dw)


def dopt_filter(hessians, rot_thr=ROT_DEGEN_THRESHOLD, trans_thr=TRANS_DEGEN_THRESHOLD):
    """(T,36) or (T,6,6) float32 LOAM Hessians -> (rot_dopt, trans_dopt, keep) like the shipped node."""
    h = np.ascontiguousarray(hessians, dtype=np.float32).reshape(-1, 36)
    n = h.shape[0]
    rot, trans, keep = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    check(_lib.lib().vf_dopt_filter_f32(h.ctypes.data_as(C.POINTER(C.c_float)), n, C.c_float(rot_thr),
                                        C.c_float(trans_thr), rot.ctypes.data_as(C.POINTER(C.c_float)),
                                        trans.ctypes.data_as(C.POINTER(C.c_float)),
                                        keep.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return rot, trans, keep.astype(bool)
