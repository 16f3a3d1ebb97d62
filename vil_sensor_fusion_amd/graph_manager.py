"""Python mirror of VILFusion::GraphManager / IMUManager over the C ABI.

Method names, argument meaning and error behaviour follow the reference
(gtsam_fusion/include/gtsam_fusion/GraphManager.h:40-96, IMUManager.h:22-27) so that the
reference's own test timelines (gtsam_fusion/test/UnitTests.cpp) read the same here.  Poses are
(q_wxyz, t) tuples instead of gtsam::Pose3; noise is a 6x6 covariance in Pose3 tangent order
[rot, trans] (what SensorManagerRos.cpp:99 wraps into noiseModel::Gaussian::Covariance).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import robust as robust_losses
from ._lib import check

# gtsam_fusion/config/carla/fusion_params.yaml:22-27
CARLA_IMU = dict(acc=1e-6, gyro=1e-6, integration=1e-8, bias_acc=1e-4, bias_omega=1e-6,
                 bias_acc_omega_int=1e-4)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class GraphManager:
    """GraphManager(imuManager): the IMU manager is folded in (addIMUMeasurement)."""

    def __init__(self, imu_params=CARLA_IMU, capacity=4096, lag=0, iterations=5, device=0,
                 prior_sigma=None, rel_tol=None, abs_tol=None, reference_compat=False, relin_threshold=None,
                 cold_start=False, fixed_capacity=False, incremental=False, wildfire=None, min_model_fidelity=None,
                 synchronous_staging=False, max_far_factors=None, far_covariance=False, robust_far=False):
        """iterations: LM trials per solve at most; a solve stops earlier once a trial changes the cost by <= abs_tol or
        <= rel_tol * cost (defaults 1e-5 / 1e-5, gtsam::LevenbergMarquardtParams; 0 / 0: always `iterations` trials)."""
        self._l = _lib.lib()
        p = _lib.ImuParamsC(imu_params["acc"], imu_params["gyro"], imu_params["integration"],
                            imu_params["bias_acc"], imu_params["bias_omega"],
                            imu_params["bias_acc_omega_int"])
        o = _lib.GraphOptsC()
        self._l.vf_graph_default_opts(C.byref(o))
        o.capacity, o.lag, o.iterations, o.device = capacity, lag, iterations, device
        if prior_sigma is not None:
            o.prior_sigma[:] = list(prior_sigma)
        if rel_tol is not None:
            o.rel_tol = rel_tol
        if abs_tol is not None:
            o.abs_tol = abs_tol
        # reference_compat: solve() = ONE iSAM2-like update (relinearizeThreshold 1e-4, GraphManager.cpp:38-43), lag must be 0
        o.reference_compat = int(bool(reference_compat))
        o.cold_start = int(bool(cold_start))      # every solve linearises all factors (tests compare it with the warm start)
        o.fixed_capacity = int(bool(fixed_capacity))   # lag = 0: fail with VF_ERR_CAPACITY instead of growing the engine
        if relin_threshold is not None:
            o.relin_threshold = relin_threshold
        # incremental (with reference_compat): a solve re-eliminates only from the first keyframe that changed (vilfusion.h)
        o.incremental = int(incremental)          # (2: the incremental kernels over the whole history every time -- what tests compare with)
        if wildfire is not None:
            o.wildfire = wildfire
        o.synchronous_staging = int(bool(synchronous_staging))     # the pre-round-6 staging: same bits, slower (tests compare the two)
        if min_model_fidelity is not None:        # GTSAM's LM accept rule (LevenbergMarquardtParams::minModelFidelity = 1e-3) instead of the library's own
            o.min_model_fidelity = min_model_fidelity
        if max_far_factors is not None:           # loop closures alive at once (default = the limit, VF_MAX_FAR_LIMIT = 32)
            o.max_far_factors = max_far_factors
        # far_covariance: marginalCovariance and the covariance callbacks take loop closures alive into account (a low-rank
        # downdate) instead of refusing while one is alive
        o.far_covariance = int(bool(far_covariance))
        # robust_far: addBetweenFactor(..., robust=...) is accepted on a pair the band cannot hold (a loop closure), which then
        # carries its loss as a far factor; without it such a pair is refused (vf_set_robust_far, once the handle exists)
        self._h = C.c_void_p()
        self._robust = {}          # end key -> (loss id, k) of the robust band factors added (between_weights)
        check(self._l.vf_create(C.byref(p), C.byref(o), C.byref(self._h)))
        if robust_far:
            check(self._l.vf_set_robust_far(self._h, 1))
        self._cbs = []

    def close(self):
        if getattr(self, "_h", None):
            self._l.vf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setInitialState(self, state16):
        """extra: anchor X(0), V(0), B(0) (and the means of their priors) at state16 = q t v bias instead of
        identity / zero; only before the first reserveNode (for logs that do not start level and at rest)."""
        s = np.ascontiguousarray(state16, dtype=np.float64).reshape(16)
        check(self._l.vf_set_initial_state(self._h, _d(s)))

    # IMUManager::addIMUMeasurement
    def addIMUMeasurement(self, time, accel, gyro):
        a = np.ascontiguousarray(accel, dtype=np.float64)
        w = np.ascontiguousarray(gyro, dtype=np.float64)
        check(self._l.vf_add_imu(self._h, C.c_double(time), _d(a), _d(w)))

    def reserveNode(self, time) -> int:
        key = C.c_uint64()
        check(self._l.vf_reserve_node(self._h, C.c_double(time), C.byref(key)))
        return key.value

    def getMostRecentPoseTime(self):
        t, k = C.c_double(), C.c_uint64()
        check(self._l.vf_most_recent_pose_time(self._h, C.byref(t), C.byref(k)))
        return t.value, k.value

    def addBetweenFactor(self, previousKey, currentKey, betweenPose, noiseCovariance, robust=None):
        """robust: None (noiseModel::Gaussian::Covariance, as the reference's sensor managers build it), or a loss over that
        Gaussian (noiseModel::Robust) as ("huber", 1.345) / ("cauchy", k) / ("geman_mcclure", k) -- band factors only, unless the
        manager was made with robust_far=True, which takes it on loop closures too
        (vf_add_between_robust; robust.py has the names and the losses' arithmetic)"""
        q = np.ascontiguousarray(betweenPose[0], dtype=np.float64)
        t = np.ascontiguousarray(betweenPose[1], dtype=np.float64)
        cov = np.ascontiguousarray(noiseCovariance, dtype=np.float64).reshape(6, 6)
        loss, k = robust_losses.parse(robust)
        if loss == robust_losses.NONE:
            check(self._l.vf_add_between(self._h, C.c_uint64(previousKey), C.c_uint64(currentKey), _d(q),
                                         _d(t), _d(cov)))
            return
        check(self._l.vf_add_between_robust(self._h, C.c_uint64(previousKey), C.c_uint64(currentKey), _d(q), _d(t), _d(cov), C.c_int(loss), C.c_double(k)))
        self._robust[int(currentKey)] = (loss, k)

    def addPoseFactor(self, key, pose, cov, robust=None):
        """an absolute pose factor on `key` (PriorFactor<Pose3>; vf_add_absolute_pose): pose = (q_wxyz, t) in the graph's world frame,
        cov 6 x 6 in tangent order [rot, trans], robust as addBetweenFactor's.  The key must carry no band between factor -- reserve
        a node of its own for the fix (reserveNode(stamp)) -- and key - 1 must still be in the window."""
        q = np.ascontiguousarray(pose[0], dtype=np.float64)
        t = np.ascontiguousarray(pose[1], dtype=np.float64)
        c = np.ascontiguousarray(cov, dtype=np.float64).reshape(6, 6)
        loss, k = robust_losses.parse(robust)
        check(self._l.vf_add_absolute_pose(self._h, C.c_uint64(key), _d(q), _d(t), _d(c), C.c_int(loss), C.c_double(k)))
        if loss != robust_losses.NONE:
            self._robust[int(key)] = (loss, k)

    def addPositionFactor(self, key, position, cov, robust=None):
        """an absolute position factor on `key` (GPSFactor; vf_add_absolute_position): position in the graph's world frame, cov 3 x 3;
        the rules of addPoseFactor"""
        p = np.ascontiguousarray(position, dtype=np.float64).reshape(3)
        c = np.ascontiguousarray(cov, dtype=np.float64).reshape(3, 3)
        loss, k = robust_losses.parse(robust)
        check(self._l.vf_add_absolute_position(self._h, C.c_uint64(key), _d(p), _d(c), C.c_int(loss), C.c_double(k)))
        if loss != robust_losses.NONE:
            self._robust[int(key)] = (loss, k)

    def absolute_factors(self, key0=None, n=None):
        """kinds (_lib.ABSOLUTE_*) of the factors in the band slots of keys key0 .. key0+n-1 (defaults: the window, as factor_errors)"""
        key0, n = self._window_keys(key0, n)
        kinds = np.zeros(n, dtype=np.int32)
        check(self._l.vf_get_absolute_factors(self._h, C.c_uint64(key0), n, kinds.ctypes.data_as(C.c_void_p)))
        return kinds

    def between_weights(self, key0=None, n=None):
        """how far the last solve's optimum has down-weighted the band between factor ending at each of the keys key0 .. key0+n-1
        (defaults: the window, as factor_errors): rho'/s, the weight GTSAM's reweighting would have given it -- 1 for a Gaussian
        factor and for an inlier, towards 0 for an outlier, nan where no factor ends.  From factor_errors alone
        (robust.weight_from_error): nothing else is read from the device."""
        key0, n = self._window_keys(key0, n)
        _, eb, _ = self.factor_errors(key0, n)
        self._robust = {k: v for k, v in self._robust.items() if k >= key0}
        out = np.full(n, np.nan)
        for i in range(n):
            if eb[i] >= 0.0:
                loss, k = self._robust.get(key0 + i, (robust_losses.NONE, 0.0))
                out[i] = robust_losses.weight_from_error(loss, k, eb[i])
        return out

    def far_weights(self):
        """per nonlinear far factor (loop closure) alive after the last solve: (previousKey, currentKey, loss name, k, weight) --
        the weight rho'/s as between_weights gives it for band factors, from the factor's error alone (vf_get_far_factors:
        vf_engine_read_far_errors through robust.weight_from_error); 1 for a Gaussian closure and for an inlier"""
        n = C.c_int()
        cap = 32        # VF_MAX_FAR_LIMIT
        a, b = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        li, kk, err = np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap)
        check(self._l.vf_get_far_factors(self._h, C.byref(n), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                         li.ctypes.data_as(C.c_void_p), _d(kk), _d(err)))
        out = []
        for i in range(n.value):
            w = robust_losses.weight_from_error(int(li[i]), float(kk[i]), err[i]) if err[i] >= 0.0 else float("nan")
            out.append((int(a[i]), int(b[i]), robust_losses.NAMES[int(li[i])], float(kk[i]), w))
        return out

    def addFactor(self, key, record190):
        """GraphManager::addFactor(const CombinedImuFactor&): queue a ready-made preintegrated factor ending at `key`
        (its 190-double record) instead of cutting one from the IMU buffer."""
        r = np.ascontiguousarray(record190, dtype=np.float64).reshape(190)
        check(self._l.vf_add_imu_factor(self._h, C.c_uint64(key), _d(r)))

    def getMostRecentEstimate(self):
        """GraphManager::getMostRecentEstimate: (q_wxyz, t, v) of a member the reference never assigns (identity, zero)."""
        q, t, v = np.zeros(4), np.zeros(3), np.zeros(3)
        check(self._l.vf_get_most_recent_estimate(self._h, _d(q), _d(t), _d(v)))
        return (q, t), v

    def solve(self):
        check(self._l.vf_solve(self._h))

    def addOptimizationCallback(self, callback):
        """callback(time, q_wxyz, t, v, bias) -- GraphManager::OptimizationCallback"""
        def tramp(_user, time, q, t, v, b):
            callback(time, np.array(q[:4]), np.array(t[:3]), np.array(v[:3]), np.array(b[:6]))
        cb = _lib.CALLBACK(tramp)
        self._cbs.append(cb)
        check(self._l.vf_set_callback(self._h, cb, None))

    def addCovarianceCallback(self, callback):
        """callback(time, q_wxyz, t, v, bias, cov15x15): the optimisation callback plus the marginal covariance of the solved
        keyframe (vf_set_covariance_callback).  While one is registered every solve computes covariances."""
        def tramp(_user, time, q, t, v, b, cov):
            callback(time, np.array(q[:4]), np.array(t[:3]), np.array(v[:3]), np.array(b[:6]),
                     np.array(cov[:225]).reshape(15, 15))
        cb = _lib.COV_CALLBACK(tramp)
        self._cbs.append(cb)
        check(self._l.vf_set_covariance_callback(self._h, cb, None))

    def marginalCovariance(self, key):
        """ISAM2::marginalCovariance(X(key)): the 15x15 covariance of a solved key in the tangent order [omega, v, velocity,
        bias acc, bias gyro] (vf_get_marginal_covariance)."""
        cov = np.zeros((15, 15))
        check(self._l.vf_get_marginal_covariance(self._h, C.c_uint64(key), _d(cov)))
        return cov

    def predict(self, time, covariance=False):
        """The state at `time`, between two solves (vf_predict_state): ((q_wxyz, t), v, bias) predicted from the last solved key
        through the queued IMU factors' steps and what reserveNode(time) would cut from the IMU buffer now, which is not
        consumed; with covariance=True also the propagated 15x15 covariance (tangent order of marginalCovariance; computes the
        solve's covariances first if there are none yet).  Not from inside a callback."""
        q, t, v, b = np.zeros(4), np.zeros(3), np.zeros(3), np.zeros(6)
        cov = np.zeros((15, 15)) if covariance else None
        check(self._l.vf_predict_state(self._h, C.c_double(time), _d(q), _d(t), _d(v), _d(b), _d(cov) if covariance else None))
        return ((q, t), v, b, cov) if covariance else ((q, t), v, b)

    def gate_between(self, previousKey, currentKey, betweenPose, noiseCovariance, threshold=None):
        """The innovation test of a between factor before addBetweenFactor takes it (vf_gate_between): how many sigmas the odometry
        increment lies from where the window as solved, and the queued IMU factors up to currentKey, expect it.  Arguments as
        addBetweenFactor's; previousKey must be the last solved key or the one before it (else status "out_of_reach").  Returns a
        dict: status (a name of _lib.GATE_STATUS), rejected (nis > threshold; None: never -- 16.81 is the 99 % quantile of
        chi-square with 6 degrees of freedom, 22.46 the 99.9 % one), nis, nis_measurement, xi (6,) [rot, trans], state (16,).
        Consumes and stages nothing.  Not from inside a callback."""
        q = np.ascontiguousarray(betweenPose[0], dtype=np.float64)
        t = np.ascontiguousarray(betweenPose[1], dtype=np.float64)
        cov = np.ascontiguousarray(noiseCovariance, dtype=np.float64).reshape(6, 6)
        g = _lib.GateResultC()
        g.struct_size = C.sizeof(g)
        check(self._l.vf_gate_between(self._h, C.c_uint64(previousKey), C.c_uint64(currentKey), _d(q), _d(t), _d(cov),
                                      0.0 if threshold is None else float(threshold), C.byref(g)))
        return dict(status=_lib.GATE_STATUS[g.status], rejected=bool(g.rejected), nis=g.nis, nis_measurement=g.nis_measurement,
                    xi=np.array(g.xi[:]), state=np.array(g.state16[:]))

    def gate_closure(self, previousKey, currentKey, betweenPose, noiseCovariance, threshold=None):
        """The same test of a LOOP CLOSURE before addBetweenFactor takes it (vf_gate_closure): a between factor on two solved keys
        of the window, any distance apart, against their joint pose covariance in everything the window holds -- closures already
        made included, whatever far_covariance says.  Arguments as addBetweenFactor's; a key not solved yet or gone from the window
        gives status "out_of_reach".  Returns what gate_between returns without the predicted state (both ends are solved
        keyframes), plus joint_covariance (12, 12): [[S_aa, S_ab], [S_ba, S_bb]] of the two poses, previousKey first, tangent
        order [rot, trans].  Consumes and stages nothing.  Not from inside a callback."""
        q = np.ascontiguousarray(betweenPose[0], dtype=np.float64)
        t = np.ascontiguousarray(betweenPose[1], dtype=np.float64)
        cov = np.ascontiguousarray(noiseCovariance, dtype=np.float64).reshape(6, 6)
        g = _lib.ClosureGateResultC()
        g.struct_size = C.sizeof(g)
        joint = np.zeros((12, 12))
        check(self._l.vf_gate_closure(self._h, C.c_uint64(previousKey), C.c_uint64(currentKey), _d(q), _d(t), _d(cov),
                                      0.0 if threshold is None else float(threshold), C.byref(g), _d(joint)))
        return dict(status=_lib.GATE_STATUS[g.status], rejected=bool(g.rejected), nis=g.nis, nis_measurement=g.nis_measurement,
                    xi=np.array(g.xi[:]), joint_covariance=joint)

    def degeneracy_scores(self, metric, subsets=("all", "trans", "rot"), information=False, key0=None, n=None):
        """One degeneracy metric (a name of degeneracy.ALL_METRICS) on `subsets` of the nav_msgs pose covariance (or,
        information=True, its inverse) of the solved keys key0 .. key0+n-1, computed on the device from the covariances of the
        last solve (vf_get_degeneracy_scores): {subset: (n,)}.  The window is one time series, the score of its oldest key is 0.
        Defaults: from the oldest key of the last solve's window to the last reserved key (which that solve must have covered)."""
        from . import degeneracy
        if key0 is None or n is None:
            last = self.getMostRecentPoseTime()[1]
            first = last - self.solverInfo()[0] + 1
            key0 = first if key0 is None else key0
            n = last - key0 + 1 if n is None else n
        rows = sorted({degeneracy.SUBSETS[s] for s in subsets})
        out = np.zeros((len(rows), n))
        check(self._l.vf_get_degeneracy_scores(self._h, _lib.SCORE_INFORMATION if information else _lib.SCORE_COVARIANCE,
                                               degeneracy._metric_id(metric), sum(1 << r for r in rows), C.c_uint64(key0), n,
                                               out.ctypes.data_as(C.c_void_p)))
        names = {v: k for k, v in degeneracy.SUBSETS.items()}
        return {names[r]: out[i] for i, r in enumerate(rows)}

    def _window_keys(self, key0, n):
        if key0 is None or n is None:
            last = self.getMostRecentPoseTime()[1]
            first = last - self.solverInfo()[0] + 1
            key0 = first if key0 is None else key0
            n = last - key0 + 1 if n is None else n
        return key0, n

    def factor_errors(self, key0=None, n=None):
        """factor->error(values) for the factors of the last solve (vf_get_factor_errors): (imu_err (n,), btw_err (n,),
        btw_prev_key (n,)) for keys key0 .. key0+n-1 -- the chi-square error 0.5 |r|^2 of the IMU factor X(key-1) -> X(key) and of
        the band between factor ending at the key, -1 where there is none, and the key that between factor starts from (-1: none).
        Defaults: the window of the last solve, as degeneracy_scores."""
        key0, n = self._window_keys(key0, n)
        ei, eb, prev = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint64)
        check(self._l.vf_get_factor_errors(self._h, C.c_uint64(key0), n, ei.ctypes.data_as(C.c_void_p), eb.ctypes.data_as(C.c_void_p),
                                           prev.ctypes.data_as(C.c_void_p)))
        return ei, eb, np.where(prev == np.iinfo(np.uint64).max, -1, prev.astype(np.int64))

    def consistency(self, thresholds=None):
        """graph.error(values) and printErrors with a threshold (vf_get_consistency): the window's summary by factor class, as
        Engine.read_consistency returns it; thresholds as Engine.factor_errors takes them (e.g. engine.CHI2_999)."""
        from . import engine
        c = _lib.ConsistencyC()
        c.struct_size = C.sizeof(c)
        check(self._l.vf_get_consistency(self._h, engine._thresholds(thresholds), C.byref(c)))
        return engine._consistency_dict(c)

    def getState(self):
        q, t, v, b = np.zeros(4), np.zeros(3), np.zeros(3), np.zeros(6)
        check(self._l.vf_get_state(self._h, _d(q), _d(t), _d(v), _d(b)))
        return (q, t), v, b

    def getBias(self):
        b = np.zeros(6)
        check(self._l.vf_get_bias(self._h, _d(b)))
        return b

    def graphSize(self):
        """graph()->size(): factors staged since the last solve (3 priors initially)."""
        s, q = C.c_int(), C.c_int()
        check(self._l.vf_graph_staged(self._h, C.byref(s), C.byref(q)))
        return s.value

    def imuQueueSize(self):
        s, q = C.c_int(), C.c_int()
        check(self._l.vf_graph_staged(self._h, C.byref(s), C.byref(q)))
        return q.value

    def lmStats(self):
        """cost after the last solve; LM trials accepted / rejected / failed since creation (diagnostics)."""
        c = C.c_double()
        a, r, f = C.c_int(), C.c_int(), C.c_int()
        check(self._l.vf_graph_lm_stats(self._h, C.byref(c), C.byref(a), C.byref(r), C.byref(f)))
        return dict(cost=c.value, accepted=a.value, rejected=r.value, solve_failures=f.value)

    def solverInfo(self):
        """(keyframes in the window of the last solve, refinement corrections per solve now, provisional LM trials so far)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._l.vf_graph_solver_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def graph(self):
        """GraphManager::graph() (GraphManager.cpp:46-49): the staged factors as a list of dicts -- kind ("prior_pose" |
        "prior_velocity" | "prior_bias" | "between" | "absolute_pose" | "absolute_position", the last two on one key given twice), keys, measured (q_wxyz, t), covariance (6 x 6), robust (None, or (loss name, k): noiseModel::Robust)."""
        n = self.graphSize()
        names = ("prior_pose", "prior_velocity", "prior_bias", "between", "absolute_pose", "absolute_position")
        out = []
        for i in range(n):
            kind, k1, k2 = C.c_int(), C.c_uint64(), C.c_uint64()
            q, t, cov = np.zeros(4), np.zeros(3), np.zeros((6, 6))
            check(self._l.vf_graph_get_staged(self._h, i, C.byref(kind), C.byref(k1), C.byref(k2), _d(q), _d(t), _d(cov)))
            loss, k = C.c_int(), C.c_double()
            check(self._l.vf_graph_get_staged_loss(self._h, i, C.byref(loss), C.byref(k)))
            out.append(dict(kind=names[kind.value], keys=(k1.value, k2.value), measured=(q, t), covariance=cov,
                            robust=None if loss.value == robust_losses.NONE else (robust_losses.NAMES[loss.value], k.value)))
        return out

    def incrementalInfo(self):
        """incremental handles: updates so far, how many re-eliminated the whole history, the keys the last update's forward
        sweep started at / its back substitution stopped at"""
        u, f, a, b = C.c_long(), C.c_long(), C.c_uint64(), C.c_uint64()
        check(self._l.vf_graph_incremental_info(self._h, C.byref(u), C.byref(f), C.byref(a), C.byref(b)))
        return dict(updates=u.value, whole_window_updates=f.value, first_eliminated_key=a.value, last_substituted_key=b.value)

    def trajectory(self, key0, n):
        s = np.zeros((n, 16))
        check(self._l.vf_get_trajectory(self._h, C.c_uint64(key0), n, _d(s)))
        return s

    def imuFactor(self, key):
        r = np.zeros(190)
        check(self._l.vf_get_imu_factor(self._h, C.c_uint64(key), _d(r)))
        return r
