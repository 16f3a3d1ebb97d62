"""ROS-free replay of SensorManagerRos (gtsam_fusion/src/gtsam_fusion/SensorManagerRos.cpp:11-158,
include/gtsam_fusion/SensorManagerRos.h:90-103): one instance per odometry source.

Host bookkeeping only (stamp<->key matching, first-odometry gating, max_time_skip, poseDiff,
covariance selection); the factors it produces are evaluated on the GPU by the GraphManager.
`reference_compat=True` reproduces the reference's poseDiff exactly, including its world-frame
rotation delta q2*q1^-1 (SensorManagerRos.cpp:148); False uses the Pose3 between R1^T R2.
"""
from __future__ import annotations

from collections import deque

import numpy as np


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _qinv(q):
    return np.array([q[0], -q[1], -q[2], -q[3]]) / np.dot(q, q)


def _qrot(q, v):
    return _qmul(_qmul(q, np.concatenate([[0.0], v])), _qinv(q))[1:]


def ros_duration_sec(later_ns: int, earlier_ns: int) -> float:
    """(later - earlier).toSec() as roscpp computes it: the difference of two ros::Time is a ros::Duration in INTEGER
    (sec, nsec), and toSec() = sec + 1e-9 * nsec (rostime duration.h).  Matters at the boundary: stamps exactly 0.1 s apart
    give exactly the double 0.1, and `0.1 < max_time_skip` with the YAML's 0.1 is false (SensorManagerRos.cpp:47)."""
    d = int(later_ns) - int(earlier_ns)
    sec, nsec = divmod(d, 10 ** 9)
    return float(sec) + 1e-9 * float(nsec)


_TANGENT_FROM_ROS = [3, 4, 5, 0, 1, 2]      # entry k of the factor's tangent [rot, trans] in a nav_msgs (x, y, z, rx, ry, rz) covariance


class Odometry:
    """The fields of nav_msgs/Odometry the reference reads.  stamp_ns: header.stamp as integer nanoseconds (what ros::Time
    holds); when absent it is the float stamp rounded to the nanosecond (exact for simulated time, not for epoch stamps)."""

    def __init__(self, stamp, position, orientation_wxyz, twist_covariance=None, stamp_ns=None):
        self.stamp = float(stamp)
        self.stamp_ns = int(round(self.stamp * 1e9)) if stamp_ns is None else int(stamp_ns)
        self.position = np.asarray(position, dtype=np.float64)
        self.orientation = np.asarray(orientation_wxyz, dtype=np.float64)
        self.twist_covariance = None if twist_covariance is None else np.asarray(twist_covariance, dtype=np.float64).reshape(6, 6)


class SensorManager:
    def __init__(self, graph_manager, optimize_after_odom, use_odom_covariance=False,
                 covariance_linear=0.1, covariance_angular=0.1, max_time_skip=0.1, reference_compat=True,
                 noise_order_compat=True, innovation_gate=None, odom_covariance_order="reference", robust=None):
        self.gm = graph_manager
        self.optimize_after_odom = optimize_after_odom
        self.use_odom_covariance = use_odom_covariance
        self.covariance_linear = covariance_linear
        self.covariance_angular = covariance_angular
        self.max_time_skip = max_time_skip
        self.reference_compat = reference_compat
        # the reference fills the constant covariance [lin, lin, lin, ang, ang, ang] (SensorManagerRos.cpp:91-97)
        # and hands it to a factor whose tangent order is [rot, trans]: the rotation gets covariance_linear, the translation
        # covariance_angular.  True reproduces that (benign in config/carla: 0.2 / 0.2, 0.1 / 0.1; not in config/san_rafael:
        # 1e-6 / 1e-7, 1e-3 / 1e-4); False puts each where its name says.
        self.noise_order_compat = noise_order_compat
        # use_odom_covariance only.  "reference": the message's 36 values are copied as the reference copies them (:87), so a
        # covariance filled as nav_msgs says, (x, y, z, rx, ry, rz), lands on a factor whose tangent order is [rot, trans]
        # with its blocks crossed (the same SURVEY 3.5-2).  "ros": the message is read as nav_msgs says and its blocks are
        # permuted to [rot, trans]: a covariance that is not isotropic (DegeneracyGate(mode="deweight")) needs this.
        if odom_covariance_order not in ("reference", "ros"):
            raise ValueError('odom_covariance_order must be "reference" or "ros"')
        self.odom_covariance_order = odom_covariance_order
        # diagnostics kept for the caller, bounded (a node runs for hours: the last `keep` entries of each)
        keep = 4096
        self.skipped = deque(maxlen=keep)    # (previous stamp, stamp) of consecutive odometry messages the max_time_skip test refused
        self.keys_and_times = deque()
        self.last_valid_odom = None
        self.last_valid_key = None
        self.has_received_odometry = False
        self.warnings = deque(maxlen=keep)
        # Innovation gate (GraphManager.gate_between; no reference code): a chi-square threshold on the nis of every odometry
        # increment before it becomes a factor -- 16.81 is the 99 % quantile of 6 degrees of freedom, 22.46 the 99.9 % one.  An
        # increment the gate can test and rejects is not added: (stamp, (previous key, key), nis) goes to `gated`.  One it cannot
        # test (out of reach, no covariance, no solve yet, ...) is added as always and counted in `ungated`.  None (the default):
        # the gate is never called.
        self.innovation_gate = None if innovation_gate is None else float(innovation_gate)
        self.gated = deque(maxlen=keep)
        self.ungated = 0
        # Robust loss on this sensor's odometry factors (GraphManager.addBetweenFactor(robust=); robust.py): None (the default, the
        # reference's Gaussian factors), or ("huber", 1.345) and the like.  It combines with the gate, which decides first: an
        # increment the gate rejects never becomes a factor; one that passes, or that the gate could not test, gets the loss.
        from . import robust as robust_losses
        self.robust = None if robust_losses.parse(robust)[0] == robust_losses.NONE else robust_losses.parse(robust)

    # SensorManagerRos.h:91-103
    def sensorCallback(self, stamp):
        if self.has_received_odometry:
            key = self.gm.reserveNode(float(stamp))
            self.keys_and_times.append((float(stamp), key))
            return key
        return None

    # SensorManagerRos.cpp:122-158
    def poseDiff(self, before: Odometry, after: Odometry):
        dx = after.position - before.position
        dxr = _qrot(_qinv(before.orientation), dx)
        if self.reference_compat:
            qr = _qmul(after.orientation, _qinv(before.orientation))      # :148 (world-frame delta)
        else:
            qr = _qmul(_qinv(before.orientation), after.orientation)
        return qr, dxr, after.twist_covariance

    def _add_between(self, a, b, pose, cov):
        """addBetweenFactor, failing soft where the library cannot take a factor iSAM2 would (GraphManager.cpp:83-88 takes any
        pair of keys).  The library takes any pair too -- a span wider than 3 keyframes or a second factor on an end key
        becomes a "far" factor (vf_engine_set_extra_between) -- but holds at most 32 of those alive per window
        (vf_graph_opts.max_far_factors; INTEGRATION.md "Limits"): one more comes back as VF_ERR_CAPACITY and is dropped here like a missed odometry
        message (:41-45 warns and carries on the same way)."""
        from ._lib import VilFusionError
        try:
            if self.robust is not None:
                try:
                    self.gm.addBetweenFactor(a, b, pose, cov, robust=self.robust)
                    return True
                except VilFusionError as exc:
                    # VF_ERR_INVALID with this message: the band cannot hold the pair, and far factors take no loss.  (Any other
                    # VF_ERR_INVALID -- a rotation that is no quaternion, ... -- is the caller's to see, as without a loss.)
                    if exc.code != -1 or "far factors take no robust loss" not in str(exc):
                        raise
                    self.warnings.append(f"between factor ({a}, {b}) added without its robust loss: {exc}")
            self.gm.addBetweenFactor(a, b, pose, cov)
            return True
        except VilFusionError as exc:
            if exc.code != -6:                  # VF_ERR_CAPACITY: span / second factor on a key
                raise
            self.warnings.append(f"between factor ({a}, {b}) not added: {exc}")
            return False

    def _gate_rejects(self, stamp, a, b, pose, cov):
        """True: the increment a -> b failed the innovation test and must not be added"""
        from ._lib import VilFusionError
        try:
            g = self.gm.gate_between(a, b, pose, cov, self.innovation_gate)
        except VilFusionError as exc:
            self.ungated += 1
            self.warnings.append(f"between factor ({a}, {b}) not gated: {exc}")
            return False
        if g["status"] != "ok":
            self.ungated += 1
            return False
        if g["rejected"]:
            self.gated.append((stamp, (a, b), g["nis"]))
        return g["rejected"]

    # SensorManagerRos.cpp:11-120
    def odometryCallback(self, msg: Odometry):
        if not self.has_received_odometry:
            self.has_received_odometry = True
            return False
        found = None
        while self.keys_and_times and found is None:
            t, key = self.keys_and_times[0]
            if t > msg.stamp:
                break
            self.keys_and_times.popleft()
            if abs(round((t - msg.stamp) * 1e9)) < 1000000:       # :34, 1 ms in ns
                found = (t, key)
        if found is None:
            self.warnings.append(f"odometry at {msg.stamp} has no corresponding key")   # :41-45
            return False
        added = False
        # :47 -- strict "<" on a ros::Duration: a 10 Hz source with exact stamps and the YAML's max_time_skip = 0.1
        # (config/carla/fusion_params.yaml:10) never passes it
        within = self.last_valid_odom is not None and ros_duration_sec(msg.stamp_ns, self.last_valid_odom.stamp_ns) < self.max_time_skip
        if self.last_valid_odom is not None and not within:
            self.skipped.append((self.last_valid_odom.stamp, msg.stamp))
        if within:
            q, t, tw = self.poseDiff(self.last_valid_odom, msg)
            if self.use_odom_covariance and self.odom_covariance_order == "ros":
                cov_ros = tw[np.ix_(_TANGENT_FROM_ROS, _TANGENT_FROM_ROS)].copy()
            elif self.use_odom_covariance:
                cov_ros = tw.T.copy()       # std::copy into a column-major Matrix66 (:87)
            elif self.noise_order_compat:   # :91-97, filled [lin,lin,lin,ang,ang,ang] as the reference does
                cov_ros = np.diag([self.covariance_linear] * 3 + [self.covariance_angular] * 3)
            else:                           # Pose3 tangent order [rot, trans]
                cov_ros = np.diag([self.covariance_angular] * 3 + [self.covariance_linear] * 3)
            if self.innovation_gate is None or not self._gate_rejects(msg.stamp, self.last_valid_key, found[1], (q, t), cov_ros):
                added = self._add_between(self.last_valid_key, found[1], (q, t), cov_ros)
            if added and self.optimize_after_odom:
                self.gm.solve()
        self.last_valid_odom = msg
        self.last_valid_key = found[1]
        return added


class AbsoluteSensorManager:
    """A sensor that measures the platform's ABSOLUTE pose or position in the graph's world frame -- a map or relocalisation result,
    motion capture, a GPS fix in a local datum -- as the reference's sensor managers treat every measurement: a node of its own at the
    fix's stamp (reserveNode), then the factor on the key returned (GraphManager.addPoseFactor / addPositionFactor).  Such a key has an
    IMU factor and no odometry ending at it, so its band slot is free for the fix.  Lever arms and the alignment of the sensor's datum
    with the world frame are the caller's.

    kind: "pose" or "position".  covariance: used for every fix that brings none (6 x 6 in tangent order [rot, trans], or 3 x 3).
    covariance_order: SensorManager's option for a 6 x 6 covariance that comes with a fix -- "reference" takes it as it is,
    "ros" reads it as nav_msgs says, (x, y, z, rx, ry, rz), and permutes its blocks to [rot, trans].  robust: a loss for every fix
    (("huber", 1.345), ...).  A fix the graph cannot take (VF_ERR_CAPACITY, VF_ERR_BAD_KEY) is dropped with a warning, like a missed
    odometry message."""

    def __init__(self, graph_manager, kind, covariance=None, robust=None, optimize_after=False, covariance_order="reference"):
        if kind not in ("pose", "position"):
            raise ValueError('kind must be "pose" or "position"')
        if covariance_order not in ("reference", "ros"):
            raise ValueError('covariance_order must be "reference" or "ros"')
        from . import robust as robust_losses
        self.gm, self.kind, self.optimize_after, self.covariance_order = graph_manager, kind, optimize_after, covariance_order
        self.covariance = None if covariance is None else np.asarray(covariance, dtype=np.float64)
        self.robust = None if robust_losses.parse(robust)[0] == robust_losses.NONE else robust_losses.parse(robust)
        self.warnings = deque(maxlen=4096)
        self.keys_and_times = deque(maxlen=4096)

    def fixCallback(self, stamp, position, orientation_wxyz=None, covariance=None):
        """one fix: returns its key, or None if the graph could not take it"""
        from ._lib import VilFusionError
        cov = self.covariance if covariance is None else np.asarray(covariance, dtype=np.float64)
        if cov is None:
            raise ValueError("a fix without a covariance, and the manager has none")
        key = self.gm.reserveNode(float(stamp))
        try:
            if self.kind == "position":
                self.gm.addPositionFactor(key, position, cov.reshape(3, 3), robust=self.robust)
            else:
                cov = cov.reshape(6, 6)
                if covariance is not None and self.covariance_order == "ros":
                    cov = cov[np.ix_(_TANGENT_FROM_ROS, _TANGENT_FROM_ROS)].copy()
                self.gm.addPoseFactor(key, (orientation_wxyz, position), cov, robust=self.robust)
        except VilFusionError as exc:
            if exc.code not in (-6, -2):
                raise
            self.warnings.append(f"absolute {self.kind} factor on key {key} not added: {exc}")
            return None
        self.keys_and_times.append((float(stamp), key))
        if self.optimize_after:
            self.gm.solve()
        return key
