"""-m gpu: an upload channel (csrc/vf_upload_channel.hpp) that grows while the previous call's copy and kernel are outstanding.

For each of vf_engine_ingest_tail, vf_engine_propagate_tail and vf_engine_gate_tail: a call with 2 raw samples per window and, with
no status or result read in between, one with 40 per window -- more than twice the first block, so the pinned block and its device
twin are both reallocated behind the first call.  What the second call leaves must be, bit for bit, what a fresh engine in the same
state leaves when it is given the second call alone.

Shape: 2 windows of capacity 64 with 8 solved keyframes each (slots 0 .. 7)."""
import functools

import numpy as np
import pytest

from tests import helpers
from vil_sensor_fusion_amd import Engine, EngineOpts, synth

pytestmark = pytest.mark.gpu

COV = synth.CARLA_IMU_COV
B, NKF, SMALL, LARGE = 2, 8, 2, 40
NO_BETWEEN = (np.full(B, -1, dtype=np.int32), np.zeros((B, 28)))
# a candidate between factor from each window's last keyframe: identity increment, unit upper-triangular square-root information
FROM_LAST = (np.full(B, NKF - 1, dtype=np.int32), np.tile(np.concatenate([[1.0], np.zeros(6), np.ones(21)]), (B, 1)))


@functools.lru_cache(maxsize=None)
def _sequence(w):
    return synth.make_sequence(seed=900 + w, n_kf=NKF + 8)


@functools.lru_cache(maxsize=None)
def _problem(oracle_mod, w):
    return helpers.build_problem(oracle_mod, _sequence(w), perturb=0.01)


def _engine(oracle, marginals):
    eng = Engine(EngineOpts(windows=B, capacity=64))
    for w in range(B):
        p = _problem(oracle, w)
        m = p["btw_b"] < NKF
        eng.set_states(w, 0, p["states"])
        eng.set_imu(w, 1, p["imu"][1:])
        eng.set_between(w, p["btw_a"][m], p["btw_b"][m], p["btw"][m])
        eng.set_prior(w, 0, p["prior"])
        eng.set_range(w, 0, NKF)
    eng.iterate(3)
    if marginals:
        eng.marginals()
    return eng


def _samples(n):
    """(step_off, steps): the n raw samples that follow each window's last keyframe"""
    lists = []
    for w in range(B):
        seq = _sequence(w)
        lists.append(seq.imu_steps[seq.imu_off[NKF]:seq.imu_off[NKF] + n])
        assert lists[-1].shape == (n, 7)
    return np.arange(B + 1, dtype=np.int32) * n, np.concatenate(lists)


def _ingest(eng, n):
    eng.ingest_tail(*_samples(n), COV, *NO_BETWEEN)


def _read_ingest(eng):
    out = np.stack([eng.get_imu(w, NKF, 1)[0] for w in range(B)])
    eng.ingest_status()             # raises what the kernels reported
    return out


def _propagate(eng, n):
    eng.propagate_tail(*_samples(n), COV, covariance=True)


def _read_propagated(eng):
    return np.stack([np.concatenate([a.ravel() for a in eng.read_propagated(w, covariance=True)]) for w in range(B)])


def _gate(eng, n):
    eng.gate_tail(*_samples(n), COV, *FROM_LAST)


def _read_gate(eng):
    status, nis = eng.read_gate_all()
    return np.concatenate([status.astype(np.float64), nis])


@pytest.mark.parametrize("call, read, marginals", [(_ingest, _read_ingest, False), (_propagate, _read_propagated, True), (_gate, _read_gate, True)],
                         ids=["ingest", "propagate", "gate"])
def test_block_grown_behind_an_outstanding_call(oracle, call, read, marginals):
    eng, fresh = _engine(oracle, marginals), _engine(oracle, marginals)
    call(eng, SMALL)
    call(eng, LARGE)                # nothing read in between: the first call's copy and kernel may still be on their way
    got = read(eng)
    call(fresh, LARGE)
    want = read(fresh)
    print(call.__name__, "differing words:", int(np.sum(got.view(np.uint64) != want.view(np.uint64))), "of", got.size, "first words:", got.ravel()[:8])
    assert np.all(np.isfinite(got)) and np.any(got != 0.0)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    eng.close()
    fresh.close()
