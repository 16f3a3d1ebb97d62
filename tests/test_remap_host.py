"""CPU: what carries a remapped covariance and needs no device -- SensorManager's odom_covariance_order, the gate's modes and
thresholds, and vf_degeneracy_remap_batch refusing bad arguments before it looks for a device."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_sensor_manager import FakeGraphManager
from vil_sensor_fusion_amd.sensor_manager import Odometry, SensorManager


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from vil_sensor_fusion_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        g.build()
    return _lib.lib()


def _feed(sm, cov):
    sm.odometryCallback(Odometry(0.0, [0, 0, 0], [1, 0, 0, 0], cov))
    for t in (0.25, 0.5):
        sm.sensorCallback(t)
        sm.odometryCallback(Odometry(t, [t, 0, 0], [1, 0, 0, 0], cov))


def test_odom_covariance_order():
    rng = np.random.default_rng(3)
    G = rng.normal(size=(6, 6))
    cov = G @ G.T + np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])          # (x, y, z, rx, ry, rz), nothing in it isotropic
    gm = FakeGraphManager()
    _feed(SensorManager(gm, False, use_odom_covariance=True, max_time_skip=1.0), cov.ravel())
    assert len(gm.between) == 1 and gm.between[0][3].tobytes() == cov.T.copy().tobytes()             # today's verbatim copy (:87)
    gm2 = FakeGraphManager()
    _feed(SensorManager(gm2, False, use_odom_covariance=True, max_time_skip=1.0, odom_covariance_order="reference"), cov.ravel())
    assert gm2.between[0][3].tobytes() == gm.between[0][3].tobytes()
    gm3 = FakeGraphManager()
    _feed(SensorManager(gm3, False, use_odom_covariance=True, max_time_skip=1.0, odom_covariance_order="ros"), cov.ravel())
    got = gm3.between[0][3]
    P = [3, 4, 5, 0, 1, 2]
    assert got.shape == (6, 6) and got.flags["C_CONTIGUOUS"]
    for i in range(6):
        for j in range(6):
            assert got[i, j] == cov[P[i], P[j]]                    # [rot, trans] <- (x, y, z, rx, ry, rz)
    assert got[0, 0] == cov[3, 3] and got[3, 3] == cov[0, 0] and got[0, 3] == cov[3, 0]
    # the constant covariance does not go through it
    gm4 = FakeGraphManager()
    _feed(SensorManager(gm4, False, covariance_linear=0.1, covariance_angular=0.01, max_time_skip=1.0, odom_covariance_order="ros"), None)
    np.testing.assert_array_equal(np.diag(gm4.between[0][3]), [0.1, 0.1, 0.1, 0.01, 0.01, 0.01])
    with pytest.raises(ValueError):
        SensorManager(gm, False, odom_covariance_order="pose3")


def test_gate_modes_and_thresholds():
    from vil_sensor_fusion_amd.degeneracy import ROT_DEGEN_THRESHOLD, TRANS_DEGEN_THRESHOLD, eigen_threshold
    from vil_sensor_fusion_amd.degeneracy_gate import DegeneracyGate
    g = DegeneracyGate()
    assert (g.mode, g.rot_thr, g.trans_thr, g.dropped, g.deweighted) == ("drop", 11.5, 28.9, 0, 0)
    with pytest.raises(ValueError):
        DegeneracyGate(mode="deweight")                            # no nominal covariance
    with pytest.raises(ValueError):
        DegeneracyGate(mode="both")
    with pytest.raises(ValueError):
        g.covariances(np.zeros((1, 36)))
    d = DegeneracyGate(mode="deweight", nominal_cov6=0.2, floor=1e-5)
    assert d.floor == 1e-5 and np.array_equal(d.nominal_cov6, np.full(6, 0.2))
    # a 3x3 block with every eigenvalue at the threshold has the log det the shipped gate tests
    for ld in (ROT_DEGEN_THRESHOLD, TRANS_DEGEN_THRESHOLD):
        assert abs(np.log(np.linalg.det(np.eye(3) * eigen_threshold(ld))) - ld) < 1e-12


def test_bad_arguments_are_refused_without_a_device(lib):
    H, nom = np.zeros((2, 36)), np.full(6, 0.1)
    H[:] = (np.eye(6) * 4e4).ravel()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(h=H, count=2, dtype=0, nom6=nom, tt=1e3, rt=1e3, floor=1e-6, order=0, cov="cov", dw="dw"):
        out = dict(cov=np.full((2, 36), 7.0), sq=np.full((2, 21), 7.0), eig=np.full((2, 6), 7.0), dw=np.full(2, 7, np.int32))
        rc = lib.vf_degeneracy_remap_batch(p(h), count, dtype, p(nom6), tt, rt, floor, order, p(out[cov] if cov else None), p(out["sq"]),
                                           p(out["eig"]), p(out[dw] if dw else None), 0, None)
        return rc, out

    zero = nom.copy()
    zero[2] = 0.0
    for kw in (dict(h=None), dict(nom6=None), dict(cov=None), dict(dw=None), dict(count=-1), dict(dtype=2), dict(order=2), dict(order=-1),
               dict(tt=0.0), dict(rt=-1.0), dict(tt=float("inf")), dict(floor=0.0), dict(floor=-1e-6), dict(floor=1.0 + 1e-12),
               dict(floor=float("nan")), dict(nom6=zero), dict(nom6=-nom)):
        rc, out = call(**kw)
        assert rc == -1, kw                                       # VF_ERR_INVALID, with a message
        assert lib.vf_last_error() not in (None, b""), kw
        assert all(np.all(a == 7) for a in out.values()), kw
    rc, out = call(count=0)
    assert rc == 0 and all(np.all(a == 7) for a in out.values())  # VF_OK without a device, nothing written
    n = C.c_int(-1)
    if not (lib.vf_device_count(C.byref(n)) == 0 and n.value > 0):
        rc, out = call()
        assert rc == -7 and all(np.all(a == 7) for a in out.values())      # VF_ERR_NO_DEVICE: no CPU path
