#!/usr/bin/env python3
"""Drop-in for the `gtsam_fusion` node (gtsam_fusion/src/gtsam_fusion_node.cpp:17-104): same private parameters
(config/carla/fusion_params.yaml: sensors/<name>/{sensor_topic, sensor_type, odom_topic, optimize_after_odom,
use_odom_covariance, covariance_linear, covariance_angular, max_time_skip}, imu/{topic, cov_*}, tf/{static_frame,
odom_frame}), same subscriptions and queue sizes, same publications (~odometry nav_msgs/Odometry + TF static_frame ->
odom_frame from the optimisation callback), behind Rovio / LOAM exactly like the reference -- the pose-graph arithmetic
runs in libvilfusion.so on the MI355X.

Extra private parameters: solver/lag (fixed-lag window in keyframes, default 1000; 0 = smooth the whole history the way the
reference's unbounded iSAM2 graph does: the engine then grows with the history (vf_engine_grow) and every solve
relinearises all of it, so a solve gets slower as the bag gets longer -- a node meant to run indefinitely keeps a lag),
solver/capacity (default lag + 192, or 4096 initial slots when lag = 0), solver/iterations, solver/rel_tol and
solver/abs_tol (LM termination, default 1e-5 / 1e-5 = gtsam's LevenbergMarquardtParams; 0 / 0 = always `iterations` trials),
solver/device, solver/initial_state (16 doubles q t v bias: the anchor X(0), V(0), B(0) and the means of their priors; default =
the reference's identity / at rest, GraphManager.cpp:20-35), reference_compat (poseDiff quirk), noise_order_compat
(constant-covariance order quirk; both default to true = what the reference does), publish_imu_rate (default
false; true: every IMU message after the first solve also publishes the state predicted at its stamp, with the propagated
covariance, as nav_msgs/Odometry on ~odometry_imu -- GraphManager.predict; ~odometry and TF stay as they are).
sensors/<name>/innovation_gate_chi2 (absent by default: no gate; a chi-square threshold, 6 degrees of freedom -- 16.81 at 99 %,
22.46 at 99.9 % -- on the innovation of every odometry increment of that sensor before it becomes a factor,
sensor_manager.SensorManager.innovation_gate).
sensors/<name>/robust_loss and robust_k (absent by default: Gaussian factors, as the reference; "huber" / "cauchy" / "geman_mcclure" and
the loss's parameter in standard deviations of the whitened residual, default robust.DEFAULT_K -- noiseModel::Robust over the
sensor's Gaussian, sensor_manager.SensorManager.robust; with innovation_gate_chi2 the gate decides first).
solver/robust_far (default false: a factor the band cannot hold -- a loop closure -- takes no loss and is added as a Gaussian factor;
true: it carries the sensor's loss as a far factor, GraphManager(robust_far=True)).
sensors/<name>/odom_covariance_order ("reference" by default: the message's twist covariance is copied as the reference copies
it; "ros": it is read as (x, y, z, rx, ry, rz) and permuted to the factor's [rot, trans] -- what a covariance
remapped by the odometry filter's ~filter/mode = deweight needs to mean what it says; use_odom_covariance only).
NOTE the default solver/lag = 1000 is a deviation: the reference smooths an unbounded iSAM2 graph (= solver/lag 0 here).

Threading: roscpp's ros::spin() runs every callback of the reference node on ONE thread (gtsam_fusion_node.cpp:101).
rospy does not: each subscription delivers on its own receive thread, and ctypes releases the GIL inside the vf_* calls.
SensorManager's bookkeeping (keys_and_times, last_valid_*) has no lock of its own -- the reference relies on that one
spinner thread -- so the node serialises its callbacks with one re-entrant lock (publish() runs inside solve(), on the
thread that holds it).

    rosrun: python3 -m vil_sensor_fusion_amd.ros.gtsam_fusion_node   (with the node's YAML loaded in its namespace,
    launch/fusion.launch:58-73)
"""
from __future__ import annotations

import threading

from ..graph_manager import GraphManager
from ..sensor_manager import Odometry, SensorManager


def odometry_from_msg(m) -> Odometry:
    """nav_msgs/Odometry -> the fields the reference reads (SensorManagerRos.cpp:122-158)"""
    p, q = m.pose.pose.position, m.pose.pose.orientation
    st = m.header.stamp
    ns = int(st.secs) * 10 ** 9 + int(st.nsecs) if hasattr(st, "secs") and hasattr(st, "nsecs") else None
    return Odometry(st.to_sec(), [p.x, p.y, p.z], [q.w, q.x, q.y, q.z], list(m.twist.covariance), stamp_ns=ns)


class FusionNode:
    """Everything of main() that is not ros::init / ros::spin, so that it can be driven by a test with stub messages."""

    def __init__(self, rospy, tf2_ros, msgs, graph_manager=None):
        """msgs: namespace with Imu, Image, PointCloud2, Odometry, TransformStamped message classes"""
        self.rospy, self.msgs = rospy, msgs
        self._lock = threading.RLock()          # one callback at a time, as under ros::spin() (gtsam_fusion_node.cpp:101)
        self._capacity_errors = 0
        P = lambda k, d=None: rospy.get_param("~" + k, d) if d is not None else rospy.get_param("~" + k)
        imu = {k: P("imu/cov_" + n) for k, n in (("acc", "accel"), ("gyro", "gyro"), ("integration", "integration"),
                                                   ("bias_acc", "bias_acc"), ("bias_omega", "bias_omega"),
                                                   ("bias_acc_omega_int", "bias_acc_omega_int"))}   # ImuManagerRos.cpp:20-33
        lag = int(P("solver/lag", 1000))
        capacity = int(P("solver/capacity", lag + 192 if lag > 0 else 4096))
        tol = lambda k: (None if rospy.get_param("~solver/" + k, -1.0) < 0 else float(rospy.get_param("~solver/" + k)))
        self.graph = graph_manager or GraphManager(imu_params=imu, capacity=capacity, lag=lag,
                                                   iterations=int(P("solver/iterations", 5)), device=int(P("solver/device", 0)),
                                                   rel_tol=tol("rel_tol"), abs_tol=tol("abs_tol"),
                                                   # loop closures / wide between factors alive at once (32, the library's default and its limit, unless set lower)
                                                   max_far_factors=(int(P("solver/max_far_factors", 0)) or None),
                                                   # covariances with loop closures alive (~publish_covariance; default false: none then)
                                                   far_covariance=bool(P("solver/far_covariance", False)),
                                                   # a sensor's robust_loss also on factors the band cannot hold (loop closures; default
                                                   # false: those are refused and the sensor manager adds them as Gaussian factors)
                                                   robust_far=bool(P("solver/robust_far", False)))
        x0 = rospy.get_param("~solver/initial_state", [])
        if graph_manager is None and len(x0) == 16:
            self.graph.setInitialState(x0)
        self.subs = [rospy.Subscriber(P("imu/topic"), msgs.Imu, queue_size=100, callback=self._serialised(self.imu_callback))]   # ImuManagerRos.cpp:11
        self.sensor_managers = {}
        compat = bool(P("reference_compat", True))
        noise_compat = bool(P("noise_order_compat", True))      # SURVEY 3.5-2 (sensor_manager.SensorManager.noise_order_compat)
        for name, cfg in sorted(P("sensors").items()):                                   # gtsam_fusion_node.cpp:32-56
            kind = cfg.get("sensor_type")
            if kind not in ("PointCloud2", "Image"):
                rospy.logwarn("Sensor %s has invalid type %s" % (name, kind))            # :52-55
                continue
            use_cov = bool(cfg["use_odom_covariance"])
            if "max_time_skip" not in cfg:
                # the reference reads it with an unchecked getParam into an uninitialised double (SensorManagerRos.h:49,85;
                # config/san_rafael/fusion_params.yaml has none): here "no limit", and a factor that an odometry gap makes
                # wider than the device's band is dropped by SensorManager._add_between
                rospy.logwarn("Sensor %s has no max_time_skip: odometry gaps are not filtered by time" % name)
            sm = SensorManager(self.graph, bool(cfg["optimize_after_odom"]), use_cov,
                               0.0 if use_cov else float(cfg["covariance_linear"]),      # SensorManagerRos.h:50-54
                               0.0 if use_cov else float(cfg["covariance_angular"]),
                               float(cfg.get("max_time_skip", float("inf"))), reference_compat=compat, noise_order_compat=noise_compat,
                               innovation_gate=cfg.get("innovation_gate_chi2"),
                               odom_covariance_order=cfg.get("odom_covariance_order", "reference"),
                               robust=None if not cfg.get("robust_loss") else
                               ((cfg["robust_loss"], float(cfg["robust_k"])) if "robust_k" in cfg else str(cfg["robust_loss"])))
            self.sensor_managers[name] = sm
            msg_type = msgs.PointCloud2 if kind == "PointCloud2" else msgs.Image
            self.subs.append(rospy.Subscriber(cfg["sensor_topic"], msg_type, queue_size=1,                    # SensorManagerRos.h:59
                                              callback=self._serialised(lambda m, sm=sm: sm.sensorCallback(m.header.stamp.to_sec()))))
            self.subs.append(rospy.Subscriber(cfg["odom_topic"], msgs.Odometry, queue_size=1,                 # :60
                                              callback=self._serialised(lambda m, sm=sm: sm.odometryCallback(odometry_from_msg(m)))))
        self.pub = rospy.Publisher("~odometry", msgs.Odometry, queue_size=1)             # gtsam_fusion_node.cpp:58
        self.broadcaster = tf2_ros.TransformBroadcaster()
        self.static_frame, self.odom_frame = P("tf/static_frame"), P("tf/odom_frame")    # :61-62
        # ~publish_covariance (no reference twin; default false: the messages stay as the reference publishes them, with zero
        # covariances): every solve computes the solved keyframe's marginal covariance and fills pose / twist covariance
        if bool(P("publish_covariance", False)):
            self.graph.addCovarianceCallback(self.publish_with_covariance)
        else:
            self.graph.addOptimizationCallback(self.publish)                             # :64
        # ~publish_imu_rate (no reference twin; default false: nothing more is advertised or published)
        self.pub_imu = rospy.Publisher("~odometry_imu", msgs.Odometry, queue_size=1) if bool(P("publish_imu_rate", False)) else None

    def _serialised(self, fn):
        """fn under the node's lock.  VF_ERR_CAPACITY from a callback (no keyframe slot left with solver/capacity fixed, or a
        window that cannot hold solver/lag plus the keyframes of one solve) does not kill the subscriber thread: it is
        logged -- the first occurrence and then every 100th, with the running count, so that a persistent failure keeps
        showing -- and the message is dropped.  (A between factor the band cannot hold never gets here:
        SensorManager._add_between handles that case.)  Every other error propagates."""
        from .._lib import VilFusionError

        def call(m):
            with self._lock:
                try:
                    return fn(m)
                except VilFusionError as exc:
                    if exc.code != -6:                      # VF_ERR_CAPACITY
                        raise
                    self._capacity_errors += 1
                    if self._capacity_errors == 1 or self._capacity_errors % 100 == 0:
                        log = getattr(self.rospy, "logerr", None) or self.rospy.logwarn
                        log("gtsam_fusion: %s (capacity error #%d: the message is dropped) -- check ~solver/lag and "
                            "~solver/capacity" % (exc, self._capacity_errors))
                    return None
        return call

    def imu_callback(self, m):                                                           # ImuManagerRos.cpp:38-52
        a, w = m.linear_acceleration, m.angular_velocity
        self.graph.addIMUMeasurement(m.header.stamp.to_sec(), [a.x, a.y, a.z], [w.x, w.y, w.z])
        if self.pub_imu is not None:
            self.publish_imu_rate(m.header.stamp.to_sec())

    def publish_imu_rate(self, time):
        """the state predicted at `time` from the last solved key, with its propagated covariance, on ~odometry_imu; nothing before
        the first solve, or for a message older than the last reserved key (VF_ERR_INVALID)"""
        from .._lib import VilFusionError
        from ..covariance import ros_pose_covariance
        try:
            (q, p), v, _bias, cov15 = self.graph.predict(time, covariance=True)
        except VilFusionError as exc:
            if exc.code != -1:
                raise
            return
        self.pub_imu.publish(self._odometry(time, q, p, v, ros_pose_covariance(q, cov15)))

    def publish_with_covariance(self, time, q, p, v, bias, cov15):
        """publish() with pose.covariance / twist.covariance from the keyframe's marginal covariance (covariance.py)"""
        from ..covariance import ros_pose_covariance
        pose36, twist36 = ros_pose_covariance(q, cov15)
        self.publish(time, q, p, v, bias, covariance=(pose36, twist36))

    def _odometry(self, time, q, p, v, covariance=None):
        stamp = self.rospy.Time.from_sec(time)
        o = self.msgs.Odometry()
        if covariance is not None:
            o.pose.covariance = [float(x) for x in covariance[0]]
            o.twist.covariance = [float(x) for x in covariance[1]]
        o.header.stamp, o.header.frame_id, o.child_frame_id = stamp, self.static_frame, self.odom_frame
        o.pose.pose.position.x, o.pose.pose.position.y, o.pose.pose.position.z = (float(x) for x in p)
        (o.pose.pose.orientation.w, o.pose.pose.orientation.x, o.pose.pose.orientation.y,
         o.pose.pose.orientation.z) = (float(x) for x in q)
        o.twist.twist.linear.x, o.twist.twist.linear.y, o.twist.twist.linear.z = (float(x) for x in v)
        return o

    def publish(self, time, q, p, v, bias, covariance=None):                             # gtsam_fusion_node.cpp:64-98
        stamp = self.rospy.Time.from_sec(time)
        self.pub.publish(self._odometry(time, q, p, v, covariance))
        t = self.msgs.TransformStamped()
        t.header.stamp, t.header.frame_id, t.child_frame_id = stamp, self.static_frame, self.odom_frame
        t.transform.translation.x, t.transform.translation.y, t.transform.translation.z = (float(x) for x in p)
        (t.transform.rotation.w, t.transform.rotation.x, t.transform.rotation.y,
         t.transform.rotation.z) = (float(x) for x in q)
        self.broadcaster.sendTransform(t)


def main():
    import types

    import rospy
    import tf2_ros
    from geometry_msgs.msg import TransformStamped
    from nav_msgs.msg import Odometry as OdometryMsg
    from sensor_msgs.msg import Image, Imu, PointCloud2
    rospy.init_node("gtsam_fusion")
    FusionNode(rospy, tf2_ros, types.SimpleNamespace(Imu=Imu, Image=Image, PointCloud2=PointCloud2, Odometry=OdometryMsg,
                                                      TransformStamped=TransformStamped))
    rospy.spin()          # rospy delivers each subscription on its own thread: FusionNode serialises them (see the module docstring)


if __name__ == "__main__":
    main()
