"""Marginal covariances, host side (no device): the nav_msgs mapping of covariance.py against a Monte-Carlo propagation
through the Pose3 retraction, the exported symbols, and argument checks that fail before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vil_sensor_fusion_amd import synth
from vil_sensor_fusion_amd.covariance import ros_pose_covariance


def _expm(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _logm(R):
    c = np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v / 2 if th < 1e-9 else th / (2 * np.sin(th)) * v


def _pose3_expmap(xi):
    """GTSAM Pose3::Expmap of [omega, v]: (Exp(omega), J_l(omega) v)"""
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        V = np.eye(3) + 0.5 * K
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    return _expm(w), V @ v


def _random_cov(rng):
    A = rng.normal(size=(15, 15))
    S = A @ A.T + 15 * np.eye(15)
    s = np.concatenate([np.full(3, 1e-3), np.full(3, 2e-2), np.full(3, 5e-2), np.full(6, 1e-3)])
    return S * np.outer(s, s) / 15


@pytest.mark.parametrize("rot", ["identity", "random"])
def test_ros_pose_covariance_against_monte_carlo(rot):
    rng = np.random.default_rng(3 if rot == "identity" else 4)
    q = np.array([1.0, 0, 0, 0]) if rot == "identity" else synth.rot_to_quat(_expm(rng.normal(size=3)))
    R = synth.quat_to_rot(q)
    t = rng.normal(size=3)
    S = _random_cov(rng)
    pose36, twist36 = ros_pose_covariance(q, S)
    # propagate samples of the 15-dof tangent through the retraction (R Exp, t + R J v) and the quaternion, then read the
    # world-frame position and rotation vector the way a nav_msgs consumer does
    L = np.linalg.cholesky(S)
    m = 200_000
    xi = rng.normal(size=(m, 15)) @ L.T
    out = np.zeros((m, 9))
    for i in range(m):
        dR, dt = _pose3_expmap(xi[i, :6])
        R1 = R @ dR
        t1 = t + R @ dt
        q1 = synth.rot_to_quat(R1)
        out[i, 0:3] = t1 - t
        out[i, 3:6] = _logm(synth.quat_to_rot(q1) @ R.T)       # world-frame rotation vector
        out[i, 6:9] = R @ xi[i, 6:9]                            # NavState velocity: v + R dv
    emp = np.cov(out.T)
    pose = np.asarray(pose36).reshape(6, 6)
    twist = np.asarray(twist36).reshape(6, 6)
    sd = np.sqrt(np.diag(emp[:6, :6]))
    err = np.abs(pose - emp[:6, :6]) / np.outer(sd, sd)
    print(rot, "pose: max normalised difference to Monte Carlo", err.max())
    assert err.max() < 0.02             # sampling error of a correlation over 2e5 samples ~ 0.005; first-order terms ~ 1e-3
    sv = np.sqrt(np.diag(emp[6:9, 6:9]))
    errv = np.abs(twist[:3, :3] - emp[6:9, 6:9]) / np.outer(sv, sv)
    assert errv.max() < 0.02
    assert np.all(twist[3:, :] == 0) and np.all(twist[:, 3:] == 0)
    assert np.allclose(pose, pose.T, rtol=0, atol=1e-18)


def test_ros_pose_covariance_identity_is_the_swap():
    S = _random_cov(np.random.default_rng(5))
    pose = np.asarray(ros_pose_covariance([1.0, 0, 0, 0], S)[0]).reshape(6, 6)
    assert np.array_equal(pose[:3, :3], S[3:6, 3:6]) and np.array_equal(pose[3:, 3:], S[0:3, 0:3])
    assert np.array_equal(pose[:3, 3:], S[3:6, 0:3])


NEW = ["vf_engine_marginals", "vf_engine_read_marginals", "vf_get_marginal_covariance", "vf_set_covariance_callback"]


def test_new_symbols_are_exported():
    from vil_sensor_fusion_amd import _lib
    import __graft_entry__ as g
    if not os.path.exists(_lib.lib_path()):
        g.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    have = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in NEW:
        assert s in have, s
        assert s in _lib.SYMBOLS, s


def test_null_handles_are_refused_without_a_device():
    from vil_sensor_fusion_amd import _lib
    l = _lib.lib()
    cov = (C.c_double * 225)()
    assert l.vf_engine_marginals(None) == -1
    assert l.vf_engine_read_marginals(None, 0, 0, 1, cov, None) == -1
    assert l.vf_get_marginal_covariance(None, C.c_uint64(1), cov) == -1
    cb = _lib.COV_CALLBACK(lambda *a: None)
    assert l.vf_set_covariance_callback(None, cb, None) == -1
    assert b"null" in l.vf_last_error()


@pytest.mark.parametrize("on", [False, True])
def test_fusion_node_publish_covariance_switch(on):
    """~publish_covariance (default false): off, the node registers the plain callback and leaves both covariance fields as the
    reference does; on, it registers the covariance callback and fills them from covariance.ros_pose_covariance"""
    import copy
    from tests.test_diagnostics_and_nodes import CARLA, _Msg, _ns, _Rospy
    from tests.test_sensor_manager import FakeGraphManager
    from vil_sensor_fusion_amd.ros.gtsam_fusion_node import FusionNode

    class GM(FakeGraphManager):
        def __init__(self):
            super().__init__()
            self.cb = self.cov_cb = None

        def addOptimizationCallback(self, cb):
            self.cb = cb

        def addCovarianceCallback(self, cb):
            self.cov_cb = cb

    params = copy.deepcopy(CARLA)
    if on:
        params["publish_covariance"] = True
    rospy, gm = _Rospy(params), GM()
    FusionNode(rospy, _ns(TransformBroadcaster=lambda: _ns(sendTransform=lambda t: None)),
               _ns(Imu="Imu", Image="Image", PointCloud2="PointCloud2", Odometry=_Msg, TransformStamped=_Msg), graph_manager=gm)
    q, p, v = np.array([0.5, 0.5, 0.5, 0.5]), np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0])
    S = _random_cov(np.random.default_rng(9))
    if not on:
        assert gm.cov_cb is None and gm.cb is not None
        gm.cb(0.1, q, p, v, np.zeros(6))
        o = rospy.pubs["~odometry"][0]
        assert "covariance" not in vars(o.pose) and "covariance" not in vars(o.twist)
        return
    assert gm.cb is None and gm.cov_cb is not None
    gm.cov_cb(0.1, q, p, v, np.zeros(6), S)
    o = rospy.pubs["~odometry"][0]
    pose36, twist36 = ros_pose_covariance(q, S)
    assert o.pose.covariance == [float(x) for x in pose36] and o.twist.covariance == [float(x) for x in twist36]
    assert (o.pose.pose.position.y, o.twist.twist.linear.z) == (2.0, 6.0)
