"""The shipped LiDAR degeneracy gate (gtsam_fusion/src/degerate_odometry_filter.cpp:29-47) over the C ABI: float32 log det
of the rotation (3,3) and translation (0,0) 3x3 blocks of the 36-float scan-matching Hessian; an odometry message is
republished only when neither is below its threshold (config/carla/fusion_params.yaml:35-36).  The arithmetic runs on
the GPU (vf_dopt_filter_f32); single messages and whole bags go through the same call.

mode="deweight" (no reference code) answers a degenerate scan with a covariance instead of a drop: covariance() /
covariances() hand the Hessians to vf_degeneracy_remap_batch, which keeps the nominal covariance in the directions the scan
observed and lets go of the others (degeneracy.remap_covariance).  Its eigenvalue thresholds are exp(threshold / 3) of the
gate's two log-det thresholds: a block with every eigenvalue there has exactly the log det the gate tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

MODES = ("drop", "deweight")


class DegeneracyGate:
    def __init__(self, rot_degen_threshold=11.5, trans_degen_threshold=28.9, mode="drop", nominal_cov6=None, floor=1e-6):
        """nominal_cov6: the nominal covariance of (x, y, z, rx, ry, rz), mode="deweight" only (one value: all six axes)"""
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        self.rot_thr, self.trans_thr = float(rot_degen_threshold), float(trans_degen_threshold)
        self.mode, self.floor = mode, float(floor)
        self.nominal_cov6 = None if nominal_cov6 is None else np.broadcast_to(np.asarray(nominal_cov6, dtype=np.float64), (6,)).copy()
        if mode == "deweight" and self.nominal_cov6 is None:
            raise ValueError('mode="deweight" needs nominal_cov6')
        self.dropped = 0
        self.deweighted = 0      # messages republished with at least one direction let go

    def evaluate(self, hessians36):
        """(n, 36) float32 -> keep (n,) bool, rot_dopt (n,), trans_dopt (n,)"""
        h = np.ascontiguousarray(hessians36, dtype=np.float32).reshape(-1, 36)
        n = h.shape[0]
        rot, trans, keep = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        check(_lib.lib().vf_dopt_filter_f32(fp(h), n, C.c_float(self.rot_thr), C.c_float(self.trans_thr), fp(rot), fp(trans),
                                            keep.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return keep.astype(bool), rot, trans

    def __call__(self, hessian36) -> bool:
        """one synchronised (odometry, OptStatus) pair: True = republish the odometry message"""
        keep, _, _ = self.evaluate(np.asarray(hessian36, dtype=np.float32).reshape(1, 36))
        if not keep[0]:
            self.dropped += 1
        return bool(keep[0])

    def covariances(self, hessians36):
        """(n, 36) float32 Hessians (what loam/OptStatus carries) -> (cov (n, 6, 6) in ROS order (x, y, z, rx, ry, rz),
        deweighted (n,)): the number of directions let go, -1 for a Hessian that is not finite -- that message counts as
        dropped, the others with a count above 0 as deweighted"""
        if self.nominal_cov6 is None:
            raise ValueError("covariances() needs nominal_cov6")
        from .degeneracy import eigen_threshold, remap_covariance
        h = np.ascontiguousarray(hessians36, dtype=np.float32).reshape(-1, 36)
        cov, _, _, dw = remap_covariance(h, self.nominal_cov6, trans_thr=eigen_threshold(self.trans_thr), rot_thr=eigen_threshold(self.rot_thr),
                                         floor=self.floor, order="loam", dtype=np.float32)
        self.dropped += int(np.sum(dw < 0))
        self.deweighted += int(np.sum(dw > 0))
        return cov, dw

    def covariance(self, hessian36):
        """one message: (cov (6, 6), deweighted)"""
        cov, dw = self.covariances(np.asarray(hessian36, dtype=np.float32).reshape(1, 36))
        return cov[0], int(dw[0])
