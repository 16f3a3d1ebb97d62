"""-m gpu: IMU-rate state prediction with propagated covariance (vf_engine_propagate_tail, k_propagate; vf_predict_state;
the node's ~odometry_imu).

Shapes: B = 3 windows of capacity 128 with 8 solved keyframes each, the last keyframes at slots 62, 63 and 64 (both sides of an
AoSoA tile edge), and a one-window engine.  Step lists from tests/pim_cases.py: "one step", "zero dt in the middle", "60 steps,
dt in [1e-4, 2e-2]", "last step interpolated, 1e-9 s", and an empty list.  The covariance bar is tests/test_propagate_mp_host's
SIGMA_BAR, fixed there on the CPU."""
import functools

import numpy as np
import pytest

from tests import helpers, pim_cases, propagate_ref
from tests import ros_stubs as R
from tests.test_propagate_mp_host import SIGMA_BAR, STATE_BAR
from vil_sensor_fusion_amd import synth
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS

pytestmark = pytest.mark.gpu

COV = synth.CARLA_IMU_COV
EPS = np.finfo(np.float64).eps
LASTS3, LASTS1 = (62, 63, 64), (63,)
NKF = 8
NO_STEPS = np.zeros((0, 7))


def steps_of(name):
    if name == "no steps":
        return NO_STEPS
    _, steps, _, cov = pim_cases.case(name)
    assert cov == COV
    return steps


def pack(lists):
    off = np.concatenate([[0], np.cumsum([len(s) for s in lists])]).astype(np.int32)
    return off, (np.concatenate(lists) if off[-1] else NO_STEPS)


@functools.lru_cache(maxsize=None)
def _problem(oracle_mod, w, last):
    seq = synth.make_sequence(seed=500 + w, n_kf=last + 3)
    prob = helpers.build_problem(oracle_mod, seq, perturb=0.01)
    lo = last - NKF + 1
    return dict(prob, lo=lo, prior=synth.prior_record(prob["states"][lo], REFERENCE_PRIOR_SIGMAS))


def make_engine(oracle, lasts, solve=True, **kw):
    """windows whose NKF keyframes end at slot `last`; the anchor prior sits on each window's first keyframe"""
    from vil_sensor_fusion_amd import Engine, EngineOpts
    eng = Engine(EngineOpts(windows=len(lasts), capacity=128, **kw))
    for w, last in enumerate(lasts):
        p = _problem(oracle, w, last)
        m = (p["btw_a"] >= p["lo"]) & (p["btw_b"] <= last)
        eng.set_states(w, 0, p["states"])
        eng.set_imu(w, 1, p["imu"][1:])
        eng.set_between(w, p["btw_a"][m], p["btw_b"][m], p["btw"][m])
        eng.set_prior(w, p["lo"], p["prior"])
        eng.set_range(w, p["lo"], last + 1)
    if solve:
        eng.iterate(3)
    return eng


def append_for_real(oracle, lasts, lists):
    """the twin: the same engine, the keyframe appended through the existing path -- ingest_tail (no between factor), slide without
    marginalisation, no further trial.  The slide moves the window's start and re-anchors the prior there; both are put back (the
    same prior record on the same first keyframe), so that the window is the solved one plus this keyframe and this factor alone.
    Returns (engine, state of the appended keyframe as the slide predicted it)."""
    twin = make_engine(oracle, lasts)
    off, steps = pack(lists)
    n = len(lasts)
    twin.ingest_tail(off, steps, COV, np.full(n, -1, dtype=np.int32), np.zeros((n, 28)))
    twin.slide(REFERENCE_PRIOR_SIGMAS, marginalize=False)
    twin.ingest_status()
    appended = [twin.get_states(w, last + 1, 1)[0] for w, last in enumerate(lasts)]
    for w, last in enumerate(lasts):
        p = _problem(oracle, w, last)
        twin.set_prior(w, p["lo"], p["prior"])
        twin.set_range(w, p["lo"], last + 2)
    return twin, appended


class World:
    """everything tests 1 - 4 compare, computed once: the solved engines, their marginals, two propagations each"""

    def __init__(self, oracle):
        self.calls = {}          # (engine name, window) -> list of dict(name, steps, x_i, sigma_ii, state, cov)
        self.twins = {}
        plan = {"b3": (LASTS3, [["one step", "no steps", "60 steps, dt in [1e-4, 2e-2]"],
                                ["zero dt in the middle", "last step interpolated, 1e-9 s", "no steps"],
                                ["no steps", "no steps", "no steps"]]),
                "b1": (LASTS1, [["last step interpolated, 1e-9 s"], ["no steps"]])}
        for key, (lasts, rounds) in plan.items():
            eng = make_engine(oracle, lasts)
            eng.marginals()
            x = [eng.get_states(w, last, 1)[0] for w, last in enumerate(lasts)]
            S = [eng.read_marginals(w, last, 1)[0] for w, last in enumerate(lasts)]
            for names in rounds:
                lists = [steps_of(n) for n in names]
                eng.propagate_tail(*pack(lists), COV, covariance=True)
                for w, name in enumerate(names):
                    st, cov = eng.read_propagated(w, covariance=True)
                    self.calls.setdefault((key, w), []).append(dict(name=name, steps=lists[w], x_i=x[w], sigma_ii=S[w], state=st, cov=cov))
            assert eng.propagate_status()[1] > 0.0
            # the states and marginals are as they were (the propagation wrote its own buffer only)
            for w, last in enumerate(lasts):
                assert np.array_equal(eng.get_states(w, last, 1)[0], x[w]) and np.array_equal(eng.read_marginals(w, last, 1)[0], S[w])
            eng.close()
            # the twin appends what the FIRST round with steps in every window propagated; b3's first round has an empty list in
            # the middle window, which ingest_tail refuses: its twin takes the middle window's steps from the second round
            first = [next(c for c in self.calls[(key, w)] if len(c["steps"])) for w in range(len(lasts))]
            twin, appended = append_for_real(oracle, lasts, [c["steps"] for c in first])
            twin.marginals()
            rows = []
            for w, last in enumerate(lasts):
                lo = _problem(oracle, w, last)["lo"]
                from tests.test_gpu_marginals import dense_H, dense_inverse
                _, cs, _ = dense_inverse(dense_H(twin.read_normal(w, lo, NKF + 1)[0]))
                new, old = twin.read_marginals(w, last + 1, 1)[0], twin.read_marginals(w, last, 1)[0]
                rows.append(dict(call=first[w], appended=appended[w], new=new, old=old, cond=cs))
            self.twins[key] = rows
            twin.close()


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


@functools.lru_cache(maxsize=None)
def _mp_reference(steps_bytes, n, x_bytes, s_bytes):
    steps = np.frombuffer(steps_bytes).reshape(n, 7)
    return propagate_ref.propagate_mp(steps, COV, np.frombuffer(x_bytes), np.frombuffer(s_bytes).reshape(15, 15))


def mp_reference(c):
    return _mp_reference(c["steps"].tobytes(), len(c["steps"]), c["x_i"].tobytes(), c["sigma_ii"].tobytes())


def test_zero_samples_are_bit_for_bit(world):
    """1: without samples the state is get_states and the covariance read_marginals of the last keyframe, bit for bit -- in the
    middle window of a batch whose neighbours have samples, at the batch's end, in every window at once, on the one-window engine"""
    seen = 0
    for (key, w), calls in world.calls.items():
        for c in calls:
            if len(c["steps"]) == 0:
                assert np.array_equal(c["state"], c["x_i"]), (key, w)
                assert np.array_equal(c["cov"], c["sigma_ii"]), (key, w)
                seen += 1
    assert seen == 6 and len(world.calls[("b3", 1)][0]["steps"]) == 0 and len(world.calls[("b3", 0)][0]["steps"]) == 1


def test_state_against_the_existing_path(world):
    """2: the same samples through ingest_tail + slide on a twin engine: the appended keyframe's state equals the propagated one to
    1e-12 per component (tests/test_gpu_parity.py's bar for k_predict)"""
    for key, rows in world.twins.items():
        for w, r in enumerate(rows):
            err = propagate_ref.state_error(r["call"]["state"], r["appended"])
            print(f"{key} window {w} ({r['call']['name']}): propagated state vs ingest_tail + slide {err:.3e}; "
                  f"bit-identical: {np.array_equal(r['call']['state'], r['appended'])}")
            assert np.all(np.isfinite(r["call"]["state"])) and err <= 1e-12, (key, w, err)
            np.testing.assert_array_equal(r["call"]["state"][10:16], r["call"]["x_i"][10:16])      # the bias is carried over


def test_covariance_against_the_mp_reference(world):
    """3: Sigma+ against tests/propagate_ref.propagate_mp fed the device's own read_marginals block, within SIGMA_BAR (fixed on the
    CPU, tests/test_propagate_mp_host.py); symmetric to the bit; the state within 1e-12 of the reference's"""
    failed = []
    for (key, w), calls in world.calls.items():
        for c in calls:
            ref = mp_reference(c)
            e, es = propagate_ref.error(c["cov"], ref["cov"]), propagate_ref.state_error(c["state"], ref["state"])
            print(f"{key} window {w} {c['name']:34s} n {len(c['steps']):3d}: Sigma+ {e:.3e} (bar {SIGMA_BAR:.2e}, ratio {e / SIGMA_BAR:.2f})  state {es:.2e}")
            assert np.array_equal(c["cov"], c["cov"].T), (key, w, c["name"])
            assert np.all(np.linalg.eigvalsh(c["cov"]) > 0)
            assert es <= STATE_BAR
            if not e <= SIGMA_BAR:
                failed.append((key, w, c["name"], e))
    assert not failed, failed


def test_meaning_the_marginal_of_the_keyframe_appended_for_real(world):
    """4: the keyframe appended for real on a twin (append_for_real), then marginals(): its Sigma is the propagated Sigma+, and the
    Sigma of the old last keyframe is what it was, both to 2 x cond x eps of the diagonally scaled H (two marginal computations,
    each within cond x eps of the truth; cond computed as tests/test_gpu_marginals.py does for its dense comparison)"""
    from tests.test_gpu_marginals import normalised_error
    for key, rows in world.twins.items():
        for w, r in enumerate(rows):
            bar = 2 * r["cond"] * EPS
            dn, do = np.diag(r["new"]), np.diag(r["old"])
            en = normalised_error(r["call"]["cov"], r["new"], dn, dn)
            eo = normalised_error(r["call"]["sigma_ii"], r["old"], do, do)
            print(f"{key} window {w} ({r['call']['name']}): propagated vs appended-for-real {en:.3e}; old last keyframe before vs after {eo:.3e}; "
                  f"bar 2 cond eps = {bar:.3e} (cond {r['cond']:.3e})")
            assert en <= bar and eo <= bar, (key, w, en, eo, bar)


@pytest.mark.parametrize("kind", ["async_one_window", "b3"])
def test_leaves_the_solve_alone(oracle, kind):
    """5: iterate(3), marginals, propagate, iterate(3): states and LM counters bit-identical to the same sequence without the
    propagate; read_result behind it gives what a fresh read gives"""
    lasts = LASTS1 if kind == "async_one_window" else LASTS3
    lists = [steps_of("60 steps, dt in [1e-4, 2e-2]"), NO_STEPS, steps_of("one step")][:len(lasts)]
    out = []
    for with_propagate in (False, True):
        e = make_engine(oracle, lasts, solve=False)
        if kind == "async_one_window":
            e.set_async(True)
        e.iterate(3)
        e.marginals()
        if with_propagate:
            e.propagate_tail(*pack(lists), COV, covariance=True)
        e.iterate(3)
        if with_propagate:
            e.propagate_tail(*pack(lists), COV, covariance=False)       # between the solve and the read of its result
        res = e.read_result(0, lasts[0])
        lo = lasts[0] - NKF + 1
        snap = [(e.get_states(w, last - NKF + 1, NKF), e.read_lm(w), e.read_delta(w, last - NKF + 1, NKF)) for w, last in enumerate(lasts)]
        np.testing.assert_array_equal(res["state"], snap[0][0][-1])
        assert (res["cost"], res["accepted"], res["rejected"], res["solve_failures"], res["device_flags"]) == \
            (snap[0][1]["cost"], snap[0][1]["accepted"], snap[0][1]["rejected"], snap[0][1]["solve_failures"], 0), lo
        if with_propagate:
            assert np.all(np.isfinite(e.read_propagated(0)))
        out.append(snap)
        e.close()
    for (s0, lm0, d0), (s1, lm1, d1) in zip(*out):
        assert np.array_equal(s0, s1) and lm0 == lm1 and np.array_equal(d0, d1)


def test_refusals(oracle):
    """6"""
    from vil_sensor_fusion_amd import Engine, EngineOpts, _lib
    from vil_sensor_fusion_amd._lib import VilFusionError

    def refused(fn, code=-1):
        with pytest.raises(VilFusionError) as ex:
            fn()
        assert ex.value.code == code, ex.value

    eng = make_engine(oracle, LASTS3)
    lists = [steps_of("one step"), NO_STEPS, steps_of("zero dt in the middle")]
    off, steps = pack(lists)
    refused(lambda: eng.read_propagated(0))                                             # a read before any propagation
    refused(lambda: eng.propagate_tail(off, steps, COV, covariance=True))              # the covariance flag without marginals
    prm = _lib.ImuParamsC(*[COV[k] for k in ("acc", "gyro", "integration", "bias_acc", "bias_omega", "bias_acc_omega_int")])
    import ctypes as C
    rc = eng._l.vf_engine_propagate_tail(eng._h, off.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), C.byref(prm), 4)
    assert rc == -1 and b"unknown flags" in eng._l.vf_last_error()                      # unknown flags
    eng.propagate_tail(off, steps, COV)                                                 # state only: works without marginals
    st = [eng.read_propagated(w) for w in range(3)]
    assert all(np.all(np.isfinite(s)) for s in st)
    np.testing.assert_array_equal(st[1], eng.get_states(1, LASTS3[1], 1)[0])
    refused(lambda: eng.read_propagated(0, covariance=True))                            # ... and has no covariance to read
    eng.marginals()
    eng.propagate_tail(off, steps, COV, covariance=True)
    assert np.all(np.isfinite(eng.read_propagated(2, covariance=True)[1]))
    eng.grow(256)
    refused(lambda: eng.read_propagated(0))                                             # a read after grow
    refused(lambda: eng.propagate_tail(off, steps, COV, covariance=True))              # (grow voids the marginals too)
    eng.propagate_tail(off, steps, COV)
    np.testing.assert_array_equal(eng.read_propagated(0), st[0])                        # the grown engine predicts the same state
    # a window with a failed factorisation: NaN covariance, finite state; its neighbours are served
    bad = eng.get_states(1, LASTS3[1] - NKF + 1, 1)
    bad[0, 4] = np.nan
    eng.set_states(1, LASTS3[1] - NKF + 1, bad)
    eng.marginals()
    eng.propagate_tail(off, steps, COV, covariance=True)
    s1, c1 = eng.read_propagated(1, covariance=True)
    assert np.all(np.isnan(c1)) and np.all(np.isfinite(s1))
    s0, c0 = eng.read_propagated(0, covariance=True)
    assert np.all(np.isfinite(c0)) and np.array_equal(s0, st[0])
    refused(lambda: eng.read_propagated(3))                                             # no such window
    eng.close()
    # a time-sharded engine
    sh = Engine(EngineOpts(windows=1, capacity=128, chunks=2))
    sh.set_shard(0, 2)
    refused(lambda: sh.propagate_tail(*pack([steps_of("one step")]), COV))
    sh.close()


# ---------------------------------------------------------------------------------------------------------------- 7: the handle
def _imu_stream(seq):
    t = synth.IMU_PHASE + np.arange(0, int((seq.kf_time[-1] + 0.5) * synth.IMU_RATE)) / synth.IMU_RATE
    traj = synth.Trajectory(seq.seed, seq.kf_time[-1] + 1.0)
    rng = np.random.default_rng([seq.seed, 0xBEEF])
    return t, traj.specific_force(t) + rng.normal(size=(t.size, 3)) * synth.IMU_NOISE, traj.body_rate(t) + rng.normal(size=(t.size, 3)) * synth.IMU_NOISE


class _Feeder:
    """feeds a GraphManager keyframe by keyframe and mirrors its IMU buffer -- what was handed in, what reserveNode has consumed --
    so that the test can cut the steps itself, by cut_imu_segment's rule"""

    def __init__(self, gm, seq, between=True):
        self.gm, self.seq, self.between = gm, seq, between
        self.t, self.acc, self.gyr = _imu_stream(seq)
        self.i, self.k, self.head, self.last_time, self.last_cut = 0, 0, 0, None, None

    def imu_until(self, time):
        while self.i < self.t.size and self.t[self.i] <= time:
            self.gm.addIMUMeasurement(self.t[self.i], self.acc[self.i], self.gyr[self.i])
            self.i += 1

    def keyframe(self, solve=True):
        self.k += 1
        k, seq = self.k, self.seq
        self.imu_until(seq.kf_time[k] + 0.01)
        key = self.gm.reserveNode(seq.kf_time[k])
        self.last_cut = self.cut(self.t[self.head] if self.last_time is None else self.last_time, seq.kf_time[k], consume=True)
        self.last_time = seq.kf_time[k]
        for a, b, q, t, c in zip(seq.btw_a, seq.btw_b, seq.btw_q, seq.btw_t, seq.btw_cov):
            if self.between and b == k and a >= 1:
                self.gm.addBetweenFactor(int(a), int(b), (q, t), np.eye(6) * c)
        if solve:
            self.gm.solve()
        return key

    def cut(self, start, end, consume=False):
        """cut_imu_segment's rule on the mirror: the previous sample is zero unless one at or before `start` is still buffered"""
        prev_t, prev = start, np.zeros(6)
        j = self.head
        while j < self.i and self.t[j] <= start:
            prev = np.concatenate([self.acc[j], self.gyr[j]])
            j += 1
        steps = []
        while j < self.i and self.t[j] < end:
            steps.append(np.concatenate([[self.t[j] - prev_t], self.acc[j], self.gyr[j]]))
            prev_t, prev = self.t[j], np.concatenate([self.acc[j], self.gyr[j]])
            j += 1
        if j < self.i:
            w = (end - prev_t) / (self.t[j] - prev_t)
            cur = np.concatenate([self.acc[j], self.gyr[j]])
            steps.append(np.concatenate([[end - prev_t], w * cur + (1.0 - w) * prev]))
        if consume:
            self.head = j
        return np.array(steps).reshape(-1, 7)


def test_handle_predicts_what_the_engine_propagates(oracle):
    """7: vf_predict_state at a time past one queued, unsolved key equals Engine.propagate_tail fed the concatenated steps, bit for bit;
    the covariance is computed on demand; the zero-step case is vf_get_state / vf_get_marginal_covariance; the refusals"""
    from vil_sensor_fusion_amd import Engine, EngineOpts
    from vil_sensor_fusion_amd._lib import VilFusionError
    from vil_sensor_fusion_amd.graph_manager import CARLA_IMU, GraphManager
    n = 12
    seq = synth.make_sequence(seed=5, n_kf=n + 3)
    gm = GraphManager(capacity=128, iterations=4, lag=0)
    f = _Feeder(gm, seq, between=False)     # (IMU factors and the anchor only: every input of the engine below is the handle's, to the bit)
    with pytest.raises(VilFusionError) as ex:
        gm.predict(0.5)
    assert ex.value.code == -1                                             # before the first solve
    for _ in range(n - 1):
        f.keyframe()
    last = n - 1
    t_last = seq.kf_time[last]
    # zero steps: the solved state and its marginal (computed on demand: nobody has asked for covariances yet)
    (q, t), v, b, cov = gm.predict(t_last, covariance=True)
    (q0, t0), v0, b0 = gm.getState()
    assert np.array_equal(np.concatenate([q, t, v, b]), np.concatenate([q0, t0, v0, b0]))
    assert np.array_equal(cov, gm.marginalCovariance(last))
    with pytest.raises(VilFusionError) as ex:
        gm.predict(t_last - 1e-3)
    assert ex.value.code == -1                                             # precedes the last reserved key
    # between two keys: what reserveNode(time) would cut now, not consumed (asking twice gives the same bits)
    f.imu_until(t_last + 0.02)
    a1 = gm.predict(t_last + 0.013, covariance=True)
    a2 = gm.predict(t_last + 0.013, covariance=True)
    assert all(np.array_equal(x, y) for x, y in zip(a1[0] + a1[1:], a2[0] + a2[1:]))
    # one queued, unsolved key, then a time past it
    key = f.keyframe(solve=False)
    assert key == last + 1 and gm.imuQueueSize() == 1
    time = seq.kf_time[key] + 0.007
    steps = np.concatenate([f.last_cut, f.cut(seq.kf_time[key], time)])      # the queued factor's steps, then the cut up to `time`
    assert len(f.last_cut) >= 5 and len(steps) > len(f.last_cut)
    (q, t), v, b, cov = gm.predict(time, covariance=True)
    got = np.concatenate([q, t, v, b])
    # the engine that holds what the handle's engine holds: its states, factors and anchor (as tests/test_gpu_marginals.py does)
    st = gm.trajectory(0, n)
    imu = np.stack([gm.imuFactor(k) for k in range(1, n)])
    eng = Engine(EngineOpts(windows=1, capacity=128))
    eng.set_states(0, 0, st)
    eng.set_imu(0, 1, imu)
    anchor = np.zeros(16)
    anchor[0] = 1.0
    eng.set_prior(0, 0, synth.prior_record(anchor, REFERENCE_PRIOR_SIGMAS))
    eng.set_range(0, 0, n)
    eng.marginals()
    eng.propagate_tail(*pack([steps]), CARLA_IMU, covariance=True)
    est, ecov = eng.read_propagated(0, covariance=True)
    assert np.array_equal(eng.read_marginals(0, last, 1)[0], gm.marginalCovariance(last))      # the same Sigma_ii went in
    np.testing.assert_array_equal(got, est)
    np.testing.assert_array_equal(cov, ecov)
    eng.close()
    # the prediction consumed nothing: the solve that follows takes the queued factor as it always did
    gm.solve()
    assert gm.imuQueueSize() == 0
    np.testing.assert_array_equal(np.concatenate(gm.predict(seq.kf_time[key])[0]), np.concatenate(gm.getState()[0]))
    # a queued ready-made record has no steps
    gm.addFactor(key + 1, gm.imuFactor(key))
    with pytest.raises(VilFusionError) as ex:
        gm.predict(seq.kf_time[key] + 1.0)
    assert ex.value.code == -1 and "ready-made" in str(ex.value)
    gm.close()


def test_handle_refuses_the_covariance_while_a_far_factor_is_alive(oracle):
    """7: with cov225 the refusals of vf_get_marginal_covariance apply; the state alone is served"""
    from tests.test_gpu_marginals import _feed_handle
    from vil_sensor_fusion_amd._lib import VilFusionError
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 40
    seq = synth.make_sequence(seed=8, n_kf=n)
    gm = GraphManager(capacity=128, iterations=3, lag=0)
    _feed_handle(gm, seq, n, far=(10, 30))
    t_last = gm.getMostRecentPoseTime()[0]
    with pytest.raises(VilFusionError) as ex:
        gm.predict(t_last, covariance=True)
    assert ex.value.code == -1 and "far" in str(ex.value)
    assert np.array_equal(np.concatenate(gm.predict(t_last)[0]), np.concatenate(gm.getState()[0]))
    gm.close()


def test_reference_compat_handle_predicts_from_the_estimate(oracle):
    """7: a reference_compat handle starts from the estimate (theta (+) delta), what vf_get_state reports, not from the linearisation
    point"""
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 10
    seq = synth.make_sequence(seed=6, n_kf=n + 2)
    gm = GraphManager(capacity=128, lag=0, reference_compat=True)
    f = _Feeder(gm, seq)
    for _ in range(n - 1):
        f.keyframe()
    t_last = seq.kf_time[n - 1]
    (q, t), v, b = gm.predict(t_last)
    (q0, t0), v0, b0 = gm.getState()
    assert np.array_equal(np.concatenate([q, t, v, b]), np.concatenate([q0, t0, v0, b0]))
    np.testing.assert_array_equal(np.concatenate([q, t, v, b]), gm.trajectory(n - 1, 1)[0])
    f.imu_until(t_last + 0.02)
    (q, t), v, b, cov = gm.predict(t_last + 0.011, covariance=True)
    assert np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) > 0)
    assert 0 < np.linalg.norm(t - t0) < 1.0
    gm.close()


# ---------------------------------------------------------------------------------------------------------------- 8: the node
def _run_node(seq, publish_imu_rate, n_kf=5):
    from tests.test_gpu_ros_replay import PARAMS, _chain
    from vil_sensor_fusion_amd.ros.gtsam_fusion_node import FusionNode
    bus = R.Bus()
    params = dict(PARAMS, solver=dict(lag=64, capacity=128, iterations=3, rel_tol=0.0, abs_tol=0.0, initial_state=[float(x) for x in seq.gt_states[0]]))
    if publish_imu_rate is not None:
        params["publish_imu_rate"] = publish_imu_rate
    rp = R.Rospy(bus, "gtsam_fusion_node", params)
    node = FusionNode(rp, R.tf2_ros_for(bus), R.ns(Imu="Imu", Image="Image", PointCloud2="PointCloud2", Odometry=R.Msg, TransformStamped=R.Msg))
    rovio = _chain(seq, 0)
    expected = []                   # what GraphManager.predict gives at each IMU message, asked right behind the node

    def imu(i):
        bus.publish("/imu/fusion", R.imu_msg(R.Time.from_sec(seq.imu_t[i]), seq.imu_acc[i], seq.imu_gyro[i]))
        if publish_imu_rate:
            from vil_sensor_fusion_amd._lib import VilFusionError
            try:
                expected.append((R.Time.from_sec(seq.imu_t[i]).to_sec(), node.graph.predict(R.Time.from_sec(seq.imu_t[i]).to_sec(), covariance=True)))
            except VilFusionError as exc:
                assert exc.code == -1
    imu(0)
    i = 1
    for k in np.nonzero(seq.kf_sensor == 0)[0][:n_kf]:
        while seq.imu_t[i] <= seq.kf_time[k] + 0.01:
            imu(i)
            i += 1
        st = R.Time.from_sec(seq.kf_time[k])
        bus.publish("/cam0/image_mono", R.sensor_msg(st))
        bus.publish("/rovio/odometry", R.odometry_msg(st, rovio[int(k)][1], rovio[int(k)][0]))
    for _ in range(6):
        imu(i)
        i += 1
    node.graph.close()
    return bus, expected


def _flat(m):
    p, o, v = m.pose.pose.position, m.pose.pose.orientation, m.twist.twist.linear
    cov = list(m.pose.covariance) + list(m.twist.covariance) if isinstance(m.pose.covariance, list) else []
    return [m.header.stamp.key(), p.x, p.y, p.z, o.w, o.x, o.y, o.z, v.x, v.y, v.z] + cov


def test_node_publishes_at_imu_rate():
    """8: with ~publish_imu_rate every IMU message after the first solve yields one ~odometry_imu message whose pose is
    GraphManager.predict's and whose covariances are ros_pose_covariance of the same call; without the parameter (or with it false)
    the node publishes the topics and messages it always did"""
    from vil_sensor_fusion_amd.covariance import ros_pose_covariance
    seq = synth.make_sequence(seed=22, n_kf=12, keep_raw=True)
    runs = {flag: _run_node(seq, flag) for flag in (None, False, True)}
    base = runs[None][0]
    assert "/gtsam_fusion_node/odometry_imu" not in base.log and len(base.log["/gtsam_fusion_node/odometry"]) == 3
    for flag in (False, True):
        bus = runs[flag][0]
        assert set(bus.log) - {"/gtsam_fusion_node/odometry_imu"} == set(base.log)
        for topic in ("/gtsam_fusion_node/odometry", "/tf"):
            assert len(bus.log[topic]) == len(base.log[topic])
        for a, b in zip(bus.log["/gtsam_fusion_node/odometry"], base.log["/gtsam_fusion_node/odometry"]):
            assert _flat(a) == _flat(b)
    assert "/gtsam_fusion_node/odometry_imu" not in runs[False][0].log
    bus, expected = runs[True]
    out = bus.log["/gtsam_fusion_node/odometry_imu"]
    assert len(out) == len(expected) > 10
    first_solve = bus.log["/gtsam_fusion_node/odometry"][0].header.stamp.to_sec()
    assert out[0].header.stamp.to_sec() >= first_solve                      # nothing before the first solve
    for m, (time, ((q, t), v, b, cov)) in zip(out, expected):
        pose36, twist36 = ros_pose_covariance(q, cov)
        assert m.header.stamp.key() == R.Time.from_sec(time).key()
        assert _flat(m) == [m.header.stamp.key()] + [float(x) for x in t] + [float(x) for x in q] + [float(x) for x in v] + \
            [float(x) for x in pose36] + [float(x) for x in twist36]
        assert m.header.frame_id == "/rovio_world" and m.child_frame_id == "/gtsam_odom"
