"""CPU: sensor_manager.AbsoluteSensorManager against a stand-in graph manager -- every fix reserves a node at its stamp and puts its
factor on the key returned; SensorManager's covariance-order option; a fix the graph cannot take is dropped with a warning."""
import numpy as np
import pytest

from vil_sensor_fusion_amd._lib import VilFusionError
from vil_sensor_fusion_amd.sensor_manager import AbsoluteSensorManager


class StandIn:
    def __init__(self, refuse=None):
        self.calls, self.key, self.refuse = [], 0, refuse

    def reserveNode(self, stamp):
        self.key += 1
        self.calls.append(("reserve", stamp, self.key))
        return self.key

    def addPositionFactor(self, key, position, cov, robust=None):
        if self.refuse is not None:
            raise VilFusionError(self.refuse, "refused")
        self.calls.append(("position", key, np.asarray(position), np.asarray(cov), robust))

    def addPoseFactor(self, key, pose, cov, robust=None):
        if self.refuse is not None:
            raise VilFusionError(self.refuse, "refused")
        self.calls.append(("pose", key, pose, np.asarray(cov), robust))

    def solve(self):
        self.calls.append(("solve",))


def test_every_fix_reserves_its_node_and_lands_on_its_key():
    gm = StandIn()
    sm = AbsoluteSensorManager(gm, "position", covariance=np.eye(3) * 4.0, robust=("huber", 1.345), optimize_after=True)
    assert sm.fixCallback(1.5, [1.0, 2.0, 3.0]) == 1 and sm.fixCallback(2.5, [4.0, 5.0, 6.0], covariance=np.eye(3)) == 2
    kinds = [c[0] for c in gm.calls]
    assert kinds == ["reserve", "position", "solve", "reserve", "position", "solve"]
    assert gm.calls[0][1] == 1.5 and gm.calls[1][1] == 1 and gm.calls[4][1] == 2
    np.testing.assert_array_equal(gm.calls[1][3], np.eye(3) * 4.0)
    np.testing.assert_array_equal(gm.calls[4][3], np.eye(3))
    assert gm.calls[1][4][1] == 1.345 and list(sm.keys_and_times) == [(1.5, 1), (2.5, 2)]


def test_covariance_order_of_a_pose_fix():
    ros = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])        # nav_msgs: x, y, z, rx, ry, rz
    ros[0, 4] = ros[4, 0] = 0.5
    for order, want in (("reference", ros), ("ros", ros[np.ix_([3, 4, 5, 0, 1, 2], [3, 4, 5, 0, 1, 2])])):
        gm = StandIn()
        sm = AbsoluteSensorManager(gm, "pose", covariance=np.eye(6) * 9.0, covariance_order=order)
        sm.fixCallback(1.0, [0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0], covariance=ros)
        sm.fixCallback(2.0, [0.0, 0.0, 2.0], [1.0, 0.0, 0.0, 0.0])
        np.testing.assert_array_equal(gm.calls[1][3], want)
        np.testing.assert_array_equal(gm.calls[3][3], np.eye(6) * 9.0)      # (the manager's own covariance is in tangent order already)
        assert gm.calls[1][2][0] == [1.0, 0.0, 0.0, 0.0] and "solve" not in [c[0] for c in gm.calls]


def test_a_fix_the_graph_cannot_take_is_dropped_with_a_warning():
    for code in (-6, -2):
        sm = AbsoluteSensorManager(StandIn(refuse=code), "position", covariance=np.eye(3))
        assert sm.fixCallback(1.0, [0.0, 0.0, 0.0]) is None and len(sm.warnings) == 1 and not sm.keys_and_times
    sm = AbsoluteSensorManager(StandIn(refuse=-3), "position", covariance=np.eye(3))
    with pytest.raises(VilFusionError):
        sm.fixCallback(1.0, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        AbsoluteSensorManager(StandIn(), "velocity")
    with pytest.raises(ValueError):
        AbsoluteSensorManager(StandIn(), "pose").fixCallback(1.0, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
