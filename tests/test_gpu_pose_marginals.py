"""-m gpu: the pose marginals in nav_msgs layout that vf_engine_marginals_ex leaves on the device with VF_MARGINALS_POSE
(kernels/kpose.inc), and the degeneracy scores computed from them there (k_degeneracy_scores_windows; vf_engine_marginal_scores,
vf_get_degeneracy_scores).

The engine of most tests: 3 windows of 70, 64 and 37 keyframes in 128 slots, slid twice with marginalisation so that lo = 2 --
a series that crosses a 64-keyframe tile (its `prev` lies in the previous workgroup), exactly one tile, less than one tile,
lo != 0, several windows with different ranges.

Bars (none taken from what the code gives):
  * cov36 against covariance.ros_pose_covariance: entrywise 64 eps sqrt(d_i d_j), d the largest diagonal entry of the 3 x 3 group
    the index belongs to -- two 3 x 3 products plus the rounding of R come to about 20 eps, a margin of 3;
  * info36 against np.linalg.inv of the device's cov36, normalised by sqrt(I_ii I_jj): 50 cond_s eps, cond_s the condition
    number of the diagonally scaled matrix (<= 26 on the CPU oracle's covariances of these windows);
  * angles of pose6 within 1e-14 rad of numpy, positions to the bit;
  * scores: bit for bit what degeneracy.scores gives for the read-back records of that window alone; against the numpy oracle
    rtol 1e-7 and atol 1e-10 max|ref| (correlation_matrix_distance, 1 - a cosine that reaches 0: atol 1e-12)."""
import numpy as np
import pytest

from oracle import degeneracy_oracle as dor
from tests import helpers
from vil_sensor_fusion_amd import Engine, EngineOpts, VilFusionError, synth
from vil_sensor_fusion_amd import degeneracy as dg
from vil_sensor_fusion_amd.covariance import _rot, ros_pose_covariance

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LENS, SEEDS, SLIDES = (70, 64, 37), (40, 41, 42), 2
RANGES = [(SLIDES, n + SLIDES) for n in LENS]
SUBS3 = ("all", "trans", "rot")
SUBS9 = tuple(dg.SUBSETS)


@pytest.fixture(scope="module")
def problems(oracle):
    out = []
    for n, seed in zip(LENS, SEEDS):
        seq = synth.make_sequence(seed=seed, n_kf=n + SLIDES + 1)
        out.append((seq, helpers.build_problem(oracle, seq, perturb=0.01)))
    return out


def build_engine(problems, before_last_solve=None, **kw):
    eng = Engine(EngineOpts(windows=3, capacity=128, **kw))
    for w, (n, (_, prob)) in enumerate(zip(LENS, problems)):
        helpers.load_engine(eng, w, prob, lo=0, hi=n)
    eng.iterate(3)
    for _ in range(SLIDES):
        eng.slide(marginalize=True)
    if before_last_solve:
        before_last_solve(eng)
    eng.iterate(3)
    return eng


@pytest.fixture(scope="module")
def scored(problems):
    """the engine with its pose marginals computed, and every window's records read back once"""
    eng = build_engine(problems)
    eng.marginals(pose=True)
    rec = [eng.read_pose_marginals(w, lo, hi - lo) for w, (lo, hi) in enumerate(RANGES)]
    yield eng, rec
    eng.close()


def euler_sxyz(q):
    """tf.transformations.euler_from_quaternion (static x-y-z) of q = (w, x, y, z), away from the gimbal lock"""
    R = _rot(q)
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0])), np.arctan2(R[1, 0], R[0, 0])])


def stack(mats, pose):
    """(n, 6, 6), (n, 6) -> the (6, 6, T) and (6, 1, T) of degeneracy.scores"""
    return np.ascontiguousarray(mats.transpose(1, 2, 0)), np.ascontiguousarray(pose.T[:, None, :])


def assert_same_bits(eng, rec, ranges, metrics, subsets):
    for information in (False, True):
        for metric in metrics:
            eng.marginal_scores(metric, subsets, information=information)
            for w, (lo, hi) in enumerate(ranges):
                cov, info, pose = rec[w]
                want = dg.scores(*stack(info if information else cov, pose), metric, subsets=subsets)
                got = eng.read_marginal_scores(w, lo, hi - lo)
                assert set(got) == set(subsets)
                for s in subsets:
                    assert got[s][0] == 0.0
                    np.testing.assert_array_equal(got[s], want[s], err_msg=f"{metric}/{s}/window {w}/information {information}")


def test_matrices_and_poses(scored):
    eng, rec = scored
    worst_cov = worst_info = worst_cond = worst_ang = 0.0
    for w, (lo, hi) in enumerate(RANGES):
        n = hi - lo
        cov, info, pose = rec[w]
        S, st = eng.read_marginals(w, lo, n), eng.get_states(w, lo, n)
        assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(info, info.transpose(0, 2, 1))
        assert np.array_equal(pose[:, :3], st[:, 4:7])
        for k in range(n):
            ref = ros_pose_covariance(st[k, :4], S[k])[0].reshape(6, 6)
            d = np.repeat([ref.diagonal()[:3].max(), ref.diagonal()[3:].max()], 3)
            worst_cov = max(worst_cov, float(np.max(np.abs(cov[k] - ref) / (64 * EPS * np.sqrt(np.outer(d, d))))))
            I = np.linalg.inv(cov[k])
            sc = 1.0 / np.sqrt(cov[k].diagonal())
            cond_s = np.linalg.cond(cov[k] * np.outer(sc, sc))
            e = float(np.max(np.abs(info[k] - I) / np.sqrt(np.outer(I.diagonal(), I.diagonal()))))
            worst_info, worst_cond = max(worst_info, e / (50 * cond_s * EPS)), max(worst_cond, cond_s)
            da = pose[k, 3:] - euler_sxyz(st[k, :4])
            worst_ang = max(worst_ang, float(np.max(np.abs((da + np.pi) % (2 * np.pi) - np.pi))))
    print(f"cov36: worst error / (64 eps sqrt(d_i d_j)) = {worst_cov:.3f}; info36: worst error / (50 cond_s eps) = {worst_info:.3f}, "
          f"largest cond_s {worst_cond:.1f}; angles: worst {worst_ang:.2e} rad")
    assert worst_cov <= 1.0
    assert worst_info <= 1.0
    assert worst_ang <= 1e-14


def test_scores_are_the_bits_of_k6_on_the_window_alone(scored):
    eng, rec = scored
    assert_same_bits(eng, rec, RANGES, dg.ALL_METRICS, SUBS3)
    assert_same_bits(eng, rec, RANGES, ["d_opt", "kullback_leibler"], SUBS9)
    # an interior stretch is the slice; the read returns the last call's metric and mask
    eng.marginal_scores("e_opt_ratio", SUBS3)
    lo, hi = RANGES[0]
    whole, part = eng.read_marginal_scores(0, lo, hi - lo), eng.read_marginal_scores(0, lo + 5, 62)
    for s in SUBS3:
        np.testing.assert_array_equal(part[s], whole[s][5:67])
    # kullback_leibler_0cov is NaN as everywhere else (beyond the window's first keyframe, whose score is 0)
    eng.marginal_scores("kullback_leibler_0cov", ("all",))
    lo, hi = RANGES[2]
    y = eng.read_marginal_scores(2, lo, hi - lo)["all"]
    assert y[0] == 0.0 and np.all(np.isnan(y[1:]))


@pytest.mark.parametrize("information", [False, True])
def test_scores_against_the_numpy_oracle(scored, information):
    eng, rec = scored
    worst, missed = {}, []
    for metric in dor.METRICS:
        eng.marginal_scores(metric, SUBS3, information=information)
        for w, (lo, hi) in enumerate(RANGES):
            cov, info, pose = rec[w]
            got = eng.read_marginal_scores(w, lo, hi - lo)
            for s in SUBS3:
                ms, ps = dor.subset(info if information else cov, pose, s)
                ref = dor.evaluate(metric, ms, ps)
                atol = 1e-12 if metric == "correlation_matrix_distance" else 1e-10 * float(np.nanmax(np.abs(ref)))
                assert np.array_equal(np.isnan(got[s]), np.isnan(ref)), (metric, s, w)
                err = float(np.nanmax(np.abs(got[s] - ref) / (atol + 1e-7 * np.abs(ref))))
                worst[metric] = max(worst.get(metric, 0.0), err)
                if not err <= 1.0:
                    missed.append((metric, s, w, err))
    print("worst |got - ref| / (atol + rtol |ref|), bar 1:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert not missed, missed


def _lm(eng):
    return [eng.read_lm(w) for w in range(3)]


def test_nothing_else_moves(problems):
    asked, twin = build_engine(problems), build_engine(problems)
    asked.marginals()
    plain = [asked.read_marginals(w, lo, hi - lo, cross=True) for w, (lo, hi) in enumerate(RANGES)]
    asked.marginals(pose=True)
    asked.marginal_scores("d_opt", SUBS3)
    asked.read_marginal_scores(0, *(RANGES[0][0], 8))
    for w, (lo, hi) in enumerate(RANGES):
        c, x = asked.read_marginals(w, lo, hi - lo, cross=True)
        assert np.array_equal(c, plain[w][0]) and np.array_equal(x, plain[w][1])
    for _ in range(2):
        asked.iterate(2)
        twin.iterate(2)
    for w in range(3):
        assert np.array_equal(asked.get_states(w, 0, 128), twin.get_states(w, 0, 128))
    assert _lm(asked) == _lm(twin)
    asked.close()
    twin.close()


def _code(call, *args):
    with pytest.raises(VilFusionError) as ex:
        call(*args)
    return ex.value.code


def test_refusals(problems, oracle):
    eng = build_engine(problems)
    lo, hi = RANGES[0]
    assert _code(eng.marginal_scores, "d_opt") == -1                       # never computed
    eng.marginals()
    assert _code(eng.marginal_scores, "d_opt") == -1                       # computed without the flag
    assert _code(eng.read_pose_marginals, 0, lo, 1) == -1
    eng.marginals(pose=True)
    assert _code(eng.read_marginal_scores, 0, lo, 1) == -1                 # no scores since these marginals
    l, h = eng._l, eng._h
    assert l.vf_engine_marginal_scores(h, 2, 0, 7) == -1 and l.vf_engine_marginal_scores(h, -1, 0, 7) == -1      # source
    assert l.vf_engine_marginal_scores(h, 0, 25, 7) == -1 and l.vf_engine_marginal_scores(h, 0, -1, 7) == -1     # metric
    assert l.vf_engine_marginal_scores(h, 0, 0, 0) == -1 and l.vf_engine_marginal_scores(h, 0, 0, 512) == -1      # mask
    eng.marginal_scores("d_opt")
    assert _code(eng.read_marginal_scores, 0, lo - 1, 4) == -2
    assert _code(eng.read_marginal_scores, 0, hi - 3, 4) == -2
    assert _code(eng.read_pose_marginals, 0, hi - 3, 4) == -2
    assert _code(eng.read_marginal_scores, 3, lo, 1) == -1                 # no such window
    eng.marginals()                                                        # the flag is that of the LAST call
    assert _code(eng.read_marginal_scores, 0, lo, 1) == -1
    eng.close()
    # a compaction voids them (the records stay in the slots they were computed for)
    seq = synth.make_sequence(seed=43, n_kf=100)
    one = Engine(EngineOpts(windows=1, capacity=192))
    helpers.load_engine(one, 0, helpers.build_problem(oracle, seq, perturb=0.01), lo=64, hi=100)
    one.iterate(3)
    one.marginals(pose=True)
    one.marginal_scores("d_opt")
    assert one.read_marginal_scores(0, 64, 36)["all"][0] == 0.0
    one.compact(64)
    assert _code(one.marginal_scores, "d_opt") == -1
    assert _code(one.read_marginal_scores, 0, 0, 36) == -1
    one.close()


def test_a_grow_voids_them_and_the_next_call_brings_them_back(oracle):
    """vf_engine_grow puts new arrays behind the handle: what the covariance calls left went with the old ones, every reader
    refuses.  Computed again they are, to the bit, those of an engine created at the new capacity that holds the same problem
    at the same states (handed over, not solved for again: the form of a solve depends on the capacity, the marginals' does not)."""
    n = 40
    prob = helpers.build_problem(oracle, synth.make_sequence(seed=44, n_kf=n), perturb=0.01)
    eng = Engine(EngineOpts(windows=1, capacity=128))
    helpers.load_engine(eng, 0, prob)
    eng.iterate(3)
    eng.marginals(pose=True)
    eng.marginal_scores("d_opt")
    assert eng.read_marginal_scores(0, 0, n)["all"][0] == 0.0
    eng.grow(192)
    assert _code(eng.read_marginals, 0, 0, n) == -1
    assert _code(eng.read_pose_marginals, 0, 0, n) == -1
    assert _code(eng.marginal_scores, "d_opt") == -1
    assert _code(eng.read_marginal_scores, 0, 0, n) == -1
    ref = Engine(EngineOpts(windows=1, capacity=192))
    helpers.load_engine(ref, 0, prob)
    ref.set_states(0, 0, eng.get_states(0, 0, n))
    got = []
    for e in (eng, ref):
        e.marginals(pose=True)
        e.marginal_scores("d_opt")
        scores = e.read_marginal_scores(0, 0, n)
        got.append([*e.read_marginals(0, 0, n, cross=True), *e.read_pose_marginals(0, 0, n), *(scores[s] for s in SUBS3)])
        e.close()
    assert len(got[0]) == 8 and np.all(np.isfinite(got[0][0])) and got[0][5][0] == 0.0
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


def test_with_a_far_factor_alive(problems):
    from tests.test_gpu_far_factors import _far_record
    rec28 = _far_record(problems[0][0], 12, 60, np.random.default_rng(5))

    def add(eng):
        eng.set_extra_between(0, np.array([12], dtype=np.int32), np.array([60], dtype=np.int32), rec28[None])
    eng = build_engine(problems, before_last_solve=add)
    assert _code(eng.marginals, False, True) == -1                         # without VF_MARGINALS_FAR: refused as the plain call is
    eng.marginals(far=True, pose=True)
    rec = [eng.read_pose_marginals(w, lo, hi - lo) for w, (lo, hi) in enumerate(RANGES)]
    S = eng.read_marginals(0, *(RANGES[0][0], LENS[0]))
    st = eng.get_states(0, RANGES[0][0], LENS[0])
    ref = np.stack([ros_pose_covariance(st[k, :4], S[k])[0].reshape(6, 6) for k in range(LENS[0])])
    d = np.sqrt(np.einsum("kii->ki", ref))
    assert np.max(np.abs(rec[0][0] - ref) / np.einsum("ki,kj->kij", d, d)) < 64 * EPS       # the records are of the DOWNDATED blocks
    assert_same_bits(eng, rec, RANGES, dg.ALL_METRICS, SUBS3)
    eng.close()


class Feeder:
    """keyframes of a synthetic sequence into a GraphManager, one solve each (tests/test_gpu_marginals._feed_handle, resumable)"""

    def __init__(self, gm, seq):
        self.gm, self.seq, self.k, self.i = gm, seq, 1, 0
        self.t = synth.IMU_PHASE + np.arange(0, int((seq.kf_time[-1] + 0.5) * synth.IMU_RATE)) / synth.IMU_RATE
        traj = synth.Trajectory(seq.seed, seq.kf_time[-1] + 1.0)
        rng = np.random.default_rng([seq.seed, 0xBEEF])
        self.acc = traj.specific_force(self.t) + rng.normal(size=(self.t.size, 3)) * synth.IMU_NOISE
        self.gyr = traj.body_rate(self.t) + rng.normal(size=(self.t.size, 3)) * synth.IMU_NOISE

    def upto(self, n):
        gm, seq = self.gm, self.seq
        for k in range(self.k, n):
            while self.i < self.t.size and self.t[self.i] <= seq.kf_time[k] + 0.01:
                gm.addIMUMeasurement(self.t[self.i], self.acc[self.i], self.gyr[self.i])
                self.i += 1
            gm.reserveNode(seq.kf_time[k])
            for a, b, q, t, c in zip(seq.btw_a, seq.btw_b, seq.btw_q, seq.btw_t, seq.btw_cov):
                if b == k and a >= 1:
                    gm.addBetweenFactor(int(a), int(b), (q, t), np.eye(6) * c)
            gm.solve()
        self.k = n


def _handle_reference(gm, oldest, n):
    """the parent commit's route: covariances and states to the host, numpy, K6 on host arrays"""
    st = gm.trajectory(oldest, n)
    cov = np.stack([ros_pose_covariance(st[k, :4], gm.marginalCovariance(oldest + k))[0].reshape(6, 6) for k in range(n)])
    pose = np.hstack([st[:, 4:7], np.stack([euler_sxyz(q) for q in st[:, :4]])])
    return cov, pose


def _check_handle(gm, oldest, n):
    cov, pose = _handle_reference(gm, oldest, n)
    for information in (False, True):
        mats = np.linalg.inv(cov) if information else cov
        for metric in dg.METRICS:
            ref = dg.scores(*stack(mats, pose), metric)
            got = gm.degeneracy_scores(metric, information=information)
            for s in SUBS3:
                atol = 1e-12 if metric == "correlation_matrix_distance" else 1e-10 * float(np.nanmax(np.abs(ref[s])))
                np.testing.assert_allclose(got[s], ref[s], rtol=1e-7, atol=atol, err_msg=f"{metric}/{s}/information {information}")
    return gm.degeneracy_scores("d_opt")


def test_handle():
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n, lag = 55, 40
    seq = synth.make_sequence(seed=5, n_kf=n + 1)
    gm = GraphManager(capacity=128, iterations=4, lag=lag)
    assert _code(gm.degeneracy_scores, "d_opt", SUBS3, False, 0, 1) == -1     # before the first solve
    feed = Feeder(gm, seq)
    feed.upto(n)
    last = n - 1
    oldest = last - lag + 1
    first = _check_handle(gm, oldest, lag)
    assert first["all"].shape == (lag,) and first["all"][0] == 0.0
    part = gm.degeneracy_scores("d_opt", key0=oldest + 3, n=10)
    for s in SUBS3:
        np.testing.assert_array_equal(part[s], first[s][3:13])
    assert _code(gm.degeneracy_scores, "d_opt", SUBS3, False, oldest - 1, 4) == -2       # marginalised
    assert _code(gm.degeneracy_scores, "d_opt", SUBS3, False, last, 2) == -2             # not solved yet
    feed.upto(n + 1)                                                                      # the next solve voids them
    second = _check_handle(gm, oldest + 1, lag)
    assert not np.array_equal(second["all"][1:], first["all"][2:])
    gm.close()
