"""Preintegration inputs shared by the host and the device tests of K0's record (tests/test_pim_mp_host.py,
tests/test_gpu_k0_mp.py, tests/test_gpu_lie_edges.py).

A case is (name, steps, bias estimate, covariances): steps are rows (dt, acc xyz, gyro xyz) exactly as K0 and
vfo_pim_integrate receive them, covariances a dict with the keys of synth.CARLA_IMU_COV."""
from __future__ import annotations

import functools

import numpy as np

from vil_sensor_fusion_amd import synth

NO_INT_COV = dict(synth.CARLA_IMU_COV, bias_acc_omega_int=0.0)
USUAL_BIAS = np.array([0.05, -0.03, 0.02, 0.1, -0.08, 0.06])


def _turn(rng, n, dt, total, bhat, wobble=0.3):
    """n steps of dt turning by about `total` rad about an axis that wobbles at `wobble` rad/s round z, gyro noise 1e-3"""
    t = np.arange(n) * dt
    ax = np.stack([np.cos(wobble * t), np.sin(wobble * t), np.full(n, 2.0)], axis=1)
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    gyro = ax * (total / (n * dt)) + bhat[3:] + rng.normal(size=(n, 3)) * 1e-3
    acc = np.array([0.3, -0.2, 9.81]) + bhat[:3] + rng.normal(size=(n, 3)) * 0.5
    return np.concatenate([np.full((n, 1), dt), acc, gyro], axis=1)


def k0_segments():
    """(name, steps (dt, acc, gyro), bhat): accumulated tangent rotations that cross 0.5 rad, pass near pi and end in (pi, 2 pi)"""
    rng = np.random.default_rng(5)
    b = USUAL_BIAS
    return [("2000 steps to 5 rad, biased", _turn(rng, 2000, 0.0025, 5.0, b), b),
            ("one step", _turn(rng, 1, 0.01, 0.6, b), b),
            ("400 steps to pi - 0.01", _turn(rng, 400, 0.005, np.pi - 0.01, np.zeros(6), 0.0), np.zeros(6)),
            ("200 steps across 0.5 to 3.5", _turn(rng, 200, 0.005, 3.5, b), b)]


def _one_axis(rng, n, dt, total):
    """n steps about one fixed axis, no gyro noise: the tangent angle is the sum of the steps' angles, so it ends at `total`"""
    ax = np.array([1.0, -2.0, 2.0]) / 3.0
    gyro = np.tile(ax * (total / (n * dt)), (n, 1))
    acc = np.array([0.3, -0.2, 9.81]) + rng.normal(size=(n, 3)) * 0.5
    return np.concatenate([np.full((n, 1), dt), acc, gyro], axis=1)


def _plain(rng, dts):
    """steps of the given dts, a vehicle turning at ~0.5 rad/s"""
    n = len(dts)
    acc = np.array([0.3, -0.2, 9.81]) + rng.normal(size=(n, 3)) * 0.5
    gyro = np.array([0.1, -0.2, 0.4]) + rng.normal(size=(n, 3)) * 0.3
    return np.concatenate([np.asarray(dts, dtype=np.float64).reshape(n, 1), acc, gyro], axis=1)


def _with_zero_dt(steps, at, rng):
    """steps with a zero-dt sample inserted before row `at` (two buffered samples that share a timestamp)"""
    z = _plain(rng, [0.0])
    return np.concatenate([steps[:at], z, steps[at:]])


@functools.lru_cache(maxsize=None)
def _cases():
    from tests.test_oracle_twin import covariance_cases
    out = [(n, s, b, c) for n, s, b, c in covariance_cases()]
    out += [(n, s, b, synth.CARLA_IMU_COV) for n, s, b in k0_segments()]
    rng = np.random.default_rng(2024)
    z = np.zeros(6)
    out.append(("one axis to 2 pi - 1e-2", _one_axis(rng, 100, 0.005, 2 * np.pi - 1e-2), z, synth.CARLA_IMU_COV))
    out.append(("one axis to 2 pi - 1e-3", _one_axis(rng, 100, 0.005, 2 * np.pi - 1e-3), z, synth.CARLA_IMU_COV))
    # unwrapped: theta is never reduced, so its norm runs past 2 pi, where J_r^{-1} is singular, between two samples.  How
    # close a sample comes to 2 pi sets the conditioning (the perpendicular part of J_r^{-1} grows as 1 / (2 pi - |theta|)):
    # this one keeps cond(D P D) at 1e4; others of the same kind reach 1e8 and exceed float64's n eps by 100x in the oracle
    wob = _turn(np.random.default_rng(2024), 300, 0.005, 6.8, USUAL_BIAS, wobble=0.05)
    out.append(("wobbling axis past 2 pi", wob, USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("single step", _plain(rng, [0.005]), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("5 steps of 1e-6 s", _plain(rng, [1e-6] * 5), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("60 steps, dt in [1e-4, 2e-2]", _plain(rng, rng.uniform(1e-4, 2e-2, 60)), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("last step interpolated, 1e-9 s", _plain(rng, [0.005] * 12 + [1e-9]), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("zero dt first", _with_zero_dt(_plain(rng, [0.005] * 6), 0, rng), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("zero dt in the middle", _with_zero_dt(_plain(rng, [0.005] * 6), 3, rng), USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("bias estimate 5x", _turn(rng, 60, 0.005, 1.5, 5 * USUAL_BIAS), 5 * USUAL_BIAS, synth.CARLA_IMU_COV))
    out.append(("bias_acc_omega_int = 0", _turn(rng, 40, 0.005, 0.8, USUAL_BIAS), USUAL_BIAS, NO_INT_COV))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def cases():
    """every case: the TestTest / San Rafael / Carla noise sets of test_oracle_twin.covariance_cases, the large-angle
    segments of k0_segments, and the edges of the step sequence (single step, tiny, irregular, interpolated and zero dt)"""
    return list(_cases())


def case(name):
    for c in _cases():
        if c[0] == name:
            return c
    raise KeyError(name)
