"""-m gpu: marginal covariances with far factors alive (vf_engine_marginals_ex with VF_MARGINALS_FAR; k4_selinv_far.inc).

The band's selected inverse is downdated by the far factors' rows: Sigma = A^-1 - Z C^-1 Z^T.  Checked against a dense inverse of
the oracle's H with the far factors in it; a window without far factors keeps the bits of the band-only call; marginalising the
closures' anchors (their rows become the linear far factor) keeps the marginals of the keyframes that stay; the device-memory and
LDS forms agree to the bit; the call leaves the LM state alone; the handle's far_covariance option."""
import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_far_factors import _far_record
from tests.test_gpu_marginals import EPS, dense_H, dense_inverse, normalised_error
from vil_sensor_fusion_amd import Engine, EngineOpts, VilFusionError, synth

pytestmark = pytest.mark.gpu

FAR = [(40, 46), (20, 70), (21, 71)]


def _with_far(prob, fa, fb, rec, states):
    return dict(prob, states=states, btw_a=np.concatenate([prob["btw_a"], fa]).astype(np.int32),
                btw_b=np.concatenate([prob["btw_b"], fb]).astype(np.int32), btw=np.vstack([prob["btw"], rec]))


def _dense_from_oracle(oracle, p):
    """the full H of the oracle's window (band as wide as the widest factor), dense"""
    _, Hb, _ = helpers.oracle_window(oracle, p).assemble()
    n, w1 = Hb.shape[0], Hb.shape[1]
    H = np.zeros((15 * n, 15 * n))
    for k in range(n):
        H[15 * k:15 * k + 15, 15 * k:15 * k + 15] = Hb[k, 0]
        for d in range(1, w1):
            if k - d >= 0:
                H[15 * k:15 * k + 15, 15 * (k - d):15 * (k - d) + 15] = Hb[k, d]
                H[15 * (k - d):15 * (k - d) + 15, 15 * k:15 * k + 15] = Hb[k, d].T
    return H


def _blocks_error(cov, cross, S):
    n = cov.shape[0]
    dg = np.diag(S)
    err = 0.0
    for k in range(n):
        dk = dg[15 * k:15 * k + 15]
        err = max(err, normalised_error(cov[k], S[15 * k:15 * k + 15, 15 * k:15 * k + 15], dk, dk))
        if k + 1 < n:
            dk1 = dg[15 * (k + 1):15 * (k + 1) + 15]
            err = max(err, normalised_error(cross[k], S[15 * (k + 1):15 * (k + 1) + 15, 15 * k:15 * k + 15], dk1, dk))
    return err


def _check_window(oracle, eng, w, prob, fa, fb, rec, n, label):
    """Sigma of window w against np.linalg.inv of the oracle's dense H (far factors in it) at the engine's states.  Bar: cond * eps
    of the scaled H (test_gpu_marginals), times the cancellation the downdate brings, rho = max_i (A^-1)_ii / Sigma_ii"""
    st = eng.get_states(w, 0, n)
    Sref, cs, _ = dense_inverse(_dense_from_oracle(oracle, _with_far(prob, fa, fb, rec, st)))
    Aref, _, _ = dense_inverse(_dense_from_oracle(oracle, dict(prob, states=st)))
    rho = float(np.max(np.diag(Aref) / np.diag(Sref)))
    cov, cross = eng.read_marginals(w, 0, n, cross=True)
    err = _blocks_error(cov, cross, Sref)
    print(f"{label}, window {w} ({len(fa)} far factors): error vs the dense inverse {err:.3e}; scaled cond(H) {cs:.3e}, rho {rho:.3f}, "
          f"bar cond * eps * rho = {cs * EPS * rho:.3e}")
    assert rho >= 1.0 and err < cs * EPS * rho, (w, err)
    return rho


def test_engine_against_dense_inverse(oracle):
    n = 200
    seq = synth.make_sequence(seed=91, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.003)
    rng = np.random.default_rng(5)
    rec = np.array([_far_record(seq, a, b, rng) for a, b in FAR])
    fa, fb = np.array([a for a, _ in FAR], dtype=np.int32), np.array([b for _, b in FAR], dtype=np.int32)
    eng = Engine(EngineOpts(windows=3, capacity=n))
    for w in range(3):
        helpers.load_engine(eng, w, prob)
    eng.set_extra_between(0, fa, fb, rec)
    eng.set_extra_between(2, fa[1:], fb[1:], rec[1:])
    eng.iterate(10)
    with pytest.raises(VilFusionError) as ex:
        eng.marginals()                                      # without the flag: refused as before
    assert ex.value.code == -1
    eng.marginals(far=True)
    rho0 = _check_window(oracle, eng, 0, prob, fa, fb, rec, n, "3 x 200")
    _check_window(oracle, eng, 2, prob, fa[1:], fb[1:], rec[1:], n, "3 x 200")
    assert rho0 > 1.01                                        # the closures really shrink the covariance
    # window 1 holds no far factor: the bits of the band-only call on an engine without far factors, at the same states
    ref = Engine(EngineOpts(windows=3, capacity=n))
    for w in range(3):
        helpers.load_engine(ref, w, prob)
        ref.set_states(w, 0, eng.get_states(w, 0, n))
    ref.marginals()
    a, b = eng.read_marginals(1, 0, n, cross=True), ref.read_marginals(1, 0, n, cross=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # with the flag and no far factors: the band-only bits everywhere
    ref.marginals(far=True)
    for w in range(3):
        c = ref.read_marginals(w, 0, n, cross=True)
        ref.marginals()
        d = ref.read_marginals(w, 0, n, cross=True)
        ref.marginals(far=True)
        assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])
    eng.close()
    ref.close()


def test_far_free_window_of_an_assembling_batch_keeps_the_band_bits(oracle):
    """A 768-window engine factors with the assembling sweep.  Far factors veto that form for its solves, not for its marginals: a
    window without far factors gets the bits of the same engine without any, and the window with them matches the dense inverse"""
    n = 160
    seq = synth.make_sequence(seed=77, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.003)
    rng = np.random.default_rng(5)
    far = [(20, 70), (21, 71)]
    fa, fb = np.array([a for a, _ in far], dtype=np.int32), np.array([b for _, b in far], dtype=np.int32)
    rec = np.array([_far_record(seq, a, b, rng) for a, b in far])
    out = []
    for with_far in (False, True):
        e = Engine(EngineOpts(windows=768, capacity=n + 64))
        for w in (0, 767):
            helpers.load_engine(e, w, prob)
        assert e.solve_form() == "assembling"
        if with_far:
            e.set_extra_between(0, fa, fb, rec)
            e.marginals(far=True)
            _check_window(oracle, e, 0, prob, fa, fb, rec, n, "768 x 160")
        else:
            e.marginals()
        out.append(e.read_marginals(767, 0, n, cross=True))
        e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_marginalising_the_anchors_keeps_the_marginals(oracle):
    """The Schur complement onto the keyframes that stay preserves their marginal: after the closures' anchors are marginalised
    (their rows become the window's linear far factor) with the states held fixed, Sigma over [lo, n) equals the matching blocks
    of Sigma over [0, n) taken before, at the same linearisation point"""
    n, drop = 60, 4
    seq = synth.make_sequence(seed=93, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.003)
    rng = np.random.default_rng(7)
    closures = [(1, 40), (2, 45)]
    fa, fb = np.array([c[0] for c in closures], dtype=np.int32), np.array([c[1] for c in closures], dtype=np.int32)
    rec = np.stack([_far_record(seq, a, b, rng, cov=1e-3) for a, b in closures])
    eng = Engine(EngineOpts(windows=1, capacity=n + 64, gauge_floor=0.0))
    helpers.load_engine(eng, 0, prob)
    eng.set_extra_between(0, fa, fb, rec)
    eng.iterate(10)
    st = eng.get_states(0, 0, n)
    eng.marginals(far=True)
    c0, x0 = eng.read_marginals(0, 0, n, cross=True)
    for _ in range(drop):
        eng.linearize()                                      # (the current linearisation is at the current states: marginalise from it)
        eng.marginalize()
        eng.drop_oldest()
    assert np.array_equal(eng.get_states(0, drop, n - drop), st[drop:])
    ends = eng.get_linear_far(0)
    assert sorted(ends.tolist()) == [40, 45] and eng.get_extra_between(0)[0].size == 0
    # (the gauge floor is off by construction, gauge_floor=0.0 above: it cannot touch the prior, which is the plain Schur complement
    # at this linearisation point -- the marginals compared are those of one point)
    eng.marginals(far=True)
    c1, x1 = eng.read_marginals(0, drop, n - drop, cross=True)
    d = np.sqrt(np.einsum("kii->ki", c0[drop:]))
    e0 = np.max(np.abs(c1 - c0[drop:]) / np.einsum("ki,kj->kij", d, d))
    e1 = np.max(np.abs(x1[:-1] - x0[drop:-1]) / np.einsum("ki,kj->kij", d[1:], d[:-1]))
    _, cs, _ = dense_inverse(dense_H(eng.read_normal(0, drop, n - drop)[0]))
    print(f"Sigma over [{drop},{n}) after the marginalisation vs before: normalised difference {e0:.3e} / cross {e1:.3e}; "
          f"scaled cond of the band {cs:.3e} (bar cond * eps = {cs * EPS:.3e})")
    assert e0 < cs * EPS and e1 < cs * EPS
    eng.close()


def test_big_forms(oracle):
    """max_far_factors = 32: twelve far factors in one window (m = 72, the device-memory form) against the dense inverse; with six
    alive, the LDS form and the device-memory form (far_big_forms) give the same bits"""
    n = 120
    seq = synth.make_sequence(seed=17, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.003)
    rng = np.random.default_rng(11)
    pairs = [(10 + 4 * i, 50 + 5 * i) for i in range(12)]
    fa, fb = np.array([a for a, _ in pairs], dtype=np.int32), np.array([b for _, b in pairs], dtype=np.int32)
    rec = np.array([_far_record(seq, a, b, rng) for a, b in pairs])
    eng = Engine(EngineOpts(windows=1, capacity=n + 64, max_far_factors=32))
    helpers.load_engine(eng, 0, prob)
    eng.set_extra_between(0, fa, fb, rec)
    eng.iterate(8)
    eng.marginals(far=True)
    _check_window(oracle, eng, 0, prob, fa, fb, rec, n, "max_far_factors 32")
    st = eng.get_states(0, 0, n)
    eng.close()
    out = []
    for big in (0, 1):
        e = Engine(EngineOpts(windows=1, capacity=n + 64, max_far_factors=32, far_big_forms=big))
        helpers.load_engine(e, 0, prob)
        e.set_extra_between(0, fa[:6], fb[:6], rec[:6])
        e.set_states(0, 0, st)
        e.marginals(far=True)
        out.append(e.read_marginals(0, 0, n, cross=True))
        e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def _engine_snapshot(e, n, lo):
    return (e.get_states(0, lo, n - lo), e.read_lm(0), e.read_delta(0, lo, n - lo), e.get_extra_between(0), e.get_linear_far(0))


def test_marginals_leave_the_lm_state_alone(oracle):
    n = 100
    seq = synth.make_sequence(seed=91, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.01)
    rng = np.random.default_rng(3)
    closures = [(1, 60), (20, 80)]
    fa, fb = np.array([c[0] for c in closures], dtype=np.int32), np.array([c[1] for c in closures], dtype=np.int32)
    rec = np.stack([_far_record(seq, a, b, rng) for a, b in closures])
    out = []
    for with_marginals in (False, True):
        e = Engine(EngineOpts(windows=1, capacity=n + 64))
        helpers.load_engine(e, 0, prob)
        e.set_extra_between(0, fa, fb, rec)
        e.iterate(3)
        for _ in range(2):                                   # (1, 60) becomes the linear far factor, (20, 80) stays a far factor
            e.marginalize()
            e.drop_oldest()
        e.iterate(3)
        if with_marginals:
            e.marginals(far=True)
            assert np.all(np.isfinite(e.read_marginals(0, 2, n - 2)))
        e.iterate(3)
        out.append(_engine_snapshot(e, n, 2))
        e.close()
    (s0, lm0, d0, x0, l0), (s1, lm1, d1, x1, l1) = out
    assert l0.tolist() == [60] and x0[0].tolist() == [20]
    assert np.array_equal(s0, s1) and lm0 == lm1 and np.array_equal(d0, d1)
    assert all(np.array_equal(a, b) for a, b in zip(x0, x1)) and np.array_equal(l0, l1)


def _feed(gm, seq, n, far=None, after_solve=None):
    """tests.test_gpu_marginals._feed_handle, with a hook after every solve"""
    traj_t = synth.IMU_PHASE + np.arange(0, int((seq.kf_time[-1] + 0.5) * synth.IMU_RATE)) / synth.IMU_RATE
    traj = synth.Trajectory(seq.seed, seq.kf_time[-1] + 1.0)
    rng = np.random.default_rng([seq.seed, 0xBEEF])
    acc = traj.specific_force(traj_t) + rng.normal(size=(traj_t.size, 3)) * synth.IMU_NOISE
    gyr = traj.body_rate(traj_t) + rng.normal(size=(traj_t.size, 3)) * synth.IMU_NOISE
    i_imu = 0
    for k in range(1, n):
        while i_imu < traj_t.size and traj_t[i_imu] <= seq.kf_time[k] + 0.01:
            gm.addIMUMeasurement(traj_t[i_imu], acc[i_imu], gyr[i_imu])
            i_imu += 1
        gm.reserveNode(seq.kf_time[k])
        for a, b, q, t, c in zip(seq.btw_a, seq.btw_b, seq.btw_q, seq.btw_t, seq.btw_cov):
            if b == k and a >= 1:
                gm.addBetweenFactor(int(a), int(b), (q, t), np.eye(6) * c)
        if far is not None and k == far[1]:
            gm.addBetweenFactor(far[0], far[1], ([1.0, 0, 0, 0], np.zeros(3)), np.eye(6) * 10.0)
        gm.solve()
        if after_solve is not None:
            after_solve(k)


def test_handle_asking_for_covariances_does_not_change_the_trajectory():
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n, lag = 60, 24
    seq = synth.make_sequence(seed=8, n_kf=n)
    runs = []
    for ask in (False, True):
        gm = GraphManager(capacity=128, iterations=3, lag=lag, far_covariance=True)
        traj, covs = [], []
        if ask:
            gm.addCovarianceCallback(lambda t, q, p, v, b, cov: covs.append(cov.copy()))

        def hook(k):
            (q, t), v, b = gm.getState()
            traj.append(np.concatenate([q, t, v, b]))
            if ask:
                S = gm.marginalCovariance(k)
                assert np.array_equal(S, covs[-1])

        _feed(gm, seq, n, far=(10, 30), after_solve=hook)
        gm.close()
        runs.append((np.array(traj), covs))
    assert np.array_equal(runs[0][0], runs[1][0])            # across the closure's anchor leaving the window (key 10 leaves at 30)
    assert all(np.all(np.isfinite(c)) for c in runs[1][1])


def test_handle_far_covariance(oracle):
    from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 40
    seq = synth.make_sequence(seed=12, n_kf=n)
    # default: refused while the closure is alive (test_gpu_marginals pins it); far_covariance: the corrected covariance
    gm = GraphManager(capacity=128, iterations=4, lag=0, far_covariance=True)
    got = []
    gm.addCovarianceCallback(lambda t, q, p, v, b, cov: got.append(cov.copy()))
    _feed(gm, seq, n, far=(10, 30))
    S = np.stack([gm.marginalCovariance(k) for k in range(n)])
    assert np.array_equal(S[-1], got[-1]) and np.all(np.isfinite(S))
    assert all(np.all(np.linalg.eigvalsh(0.5 * (s + s.T)) > 0) for s in S)
    st = gm.trajectory(0, n)
    imu = np.stack([gm.imuFactor(k) for k in range(1, n)])
    gm.close()
    # a 1-window engine with the handle's factors and states
    m = seq.btw_a >= 1
    eng = Engine(EngineOpts(windows=1, capacity=128))
    eng.set_states(0, 0, st)
    eng.set_imu(0, 1, imu)
    eng.set_between(0, seq.btw_a[m], seq.btw_b[m], synth.between_records(seq)[m])
    anchor = np.zeros(16)
    anchor[0] = 1.0
    eng.set_prior(0, 0, synth.prior_record(anchor, REFERENCE_PRIOR_SIGMAS))
    eng.set_range(0, 0, n)
    far = np.zeros(28)
    far[0] = 1.0
    iu = np.triu_indices(6)
    far[7 + np.nonzero(iu[0] == iu[1])[0]] = 1.0 / np.sqrt(10.0)
    eng.set_extra_between(0, np.array([10], dtype=np.int32), np.array([30], dtype=np.int32), far[None])
    eng.marginals(far=True)
    E = eng.read_marginals(0, 0, n)
    _, cs, _ = dense_inverse(dense_H(eng.read_normal(0, 0, n)[0]))
    d = np.sqrt(np.einsum("kii->ki", E))
    diff = np.max(np.abs(S - E) / np.einsum("ki,kj->kij", d, d))
    print(f"far_covariance handle vs engine on its factors and states: max normalised difference {diff:.3e} (bar {cs * EPS:.3e})")
    assert diff < cs * EPS
    # the closure can only shrink the covariance: the same engine without it, at the same states (the handle fed the stream without
    # the closure would solve for other states, and Sigma moves with them by more than the rounding this bar is about)
    eng.set_extra_between(0, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 28)))
    eng.marginals()
    S0 = eng.read_marginals(0, 0, n)
    eng.close()
    worst = 1.0
    for k in range(n):
        dk = 1.0 / np.sqrt(np.diag(S0[k]))
        D = (S0[k] - S[k]) * np.outer(dk, dk)
        worst = min(worst, float(np.linalg.eigvalsh(0.5 * (D + D.T)).min()))
    print(f"Sigma without the closure - Sigma with it: smallest normalised eigenvalue {worst:.3e}; key 30 position trace "
          f"{np.trace(S0[30][3:6, 3:6]):.3e} -> {np.trace(S[30][3:6, 3:6]):.3e}")
    assert worst > -cs * EPS
    assert np.trace(S[30][3:6, 3:6]) < np.trace(S0[30][3:6, 3:6])
    # fixed lag, the closure's anchor gone: finite covariances from every solve; asynchronous and synchronous staging, same bits
    runs = []
    for sync in (False, True):
        gm = GraphManager(capacity=128, iterations=3, lag=24, far_covariance=True, synchronous_staging=sync)
        covs = []
        gm.addCovarianceCallback(lambda t, q, p, v, b, cov: covs.append(cov.copy()))
        _feed(gm, seq, n, far=(10, 30))
        gm.close()
        assert len(covs) == n - 1 and all(np.all(np.isfinite(c)) for c in covs)
        runs.append(np.array(covs))
    assert np.array_equal(runs[0], runs[1])
