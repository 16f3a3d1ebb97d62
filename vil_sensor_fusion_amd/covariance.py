"""Marginal covariances of solved keyframes in the layouts of nav_msgs/Odometry (host numpy, no device).

The engine reports a keyframe's 15x15 covariance in its own tangent order: [omega, v] of Pose3 -- both
in the BODY frame, since Pose3 retracts as (R Exp(omega), t + R v) -- then the velocity increment (NavState: v + R dv, body
frame), then the bias [acc, gyro].  nav_msgs/Odometry wants the pose covariance over (x, y, z, rx, ry, rz) and the twist
covariance over (vx, vy, vz, wx, wy, wz), both row-major 6x6 as 36 floats.
"""
from __future__ import annotations

import numpy as np


def _rot(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def ros_pose_covariance(q, cov15):
    """(pose36, twist36) for nav_msgs/Odometry from the 15x15 covariance of a keyframe whose rotation is q (w, x, y, z).

    Convention: both are expressed in the static (world) frame the odometry's header names.  To first order a body-frame
    perturbation (omega, v) moves the pose by R omega (rotation vector about the world axes, the (rx, ry, rz) of nav_msgs)
    and R v (position), so pose = diag(R, R) P Sigma_pose P^T diag(R, R)^T with P the swap [omega, v] -> [v, omega].  The
    velocity block maps to R Sigma_vv R^T, the (vx, vy, vz) block of the twist covariance; its angular block is not estimated
    and stays zero, as do the cross terms between linear and angular velocity."""
    S = np.asarray(cov15, dtype=np.float64).reshape(15, 15)
    R = _rot(q)
    P = np.zeros((6, 6))
    P[0:3, 3:6] = np.eye(3)
    P[3:6, 0:3] = np.eye(3)
    D = np.zeros((6, 6))
    D[0:3, 0:3] = R
    D[3:6, 3:6] = R
    A = D @ P
    pose = A @ S[0:6, 0:6] @ A.T
    twist = np.zeros((6, 6))
    twist[0:3, 0:3] = R @ S[6:9, 6:9] @ R.T
    return pose.reshape(36), twist.reshape(36)
