"""-m gpu: marginal covariances of solved keyframes (vf_engine_marginals, K4s k_band_selinv; vf_get_marginal_covariance).

Every block Sigma_kk and Sigma_{k+1,k} is checked against a dense inverse of the same undamped H (vf_engine_read_normal); the
call must leave the LM state bit for bit as it was; the one-window engine (partitioned solves) and a 768-window engine
(assembling sweep) give the same Sigma; the handle's getter and covariance callback agree."""
import numpy as np
import pytest

from tests import helpers
from vil_sensor_fusion_amd import synth

pytestmark = pytest.mark.gpu


def dense_H(Hb):
    n = Hb.shape[0]
    H = np.zeros((15 * n, 15 * n))
    for k in range(n):
        H[15 * k:15 * k + 15, 15 * k:15 * k + 15] = Hb[k, 0]
        for d in (1, 2, 3):
            if k - d >= 0:
                B = Hb[k, d]
                H[15 * k:15 * k + 15, 15 * (k - d):15 * (k - d) + 15] = B
                H[15 * (k - d):15 * (k - d) + 15, 15 * k:15 * k + 15] = B.T
    return H


def dense_inverse(H):
    """inverse after symmetric diagonal scaling (the spread of H's diagonal is most of its condition number)"""
    d = 1.0 / np.sqrt(np.diag(H))
    Hs = H * np.outer(d, d)
    return np.linalg.inv(Hs) * np.outer(d, d), np.linalg.cond(Hs), np.linalg.cond(H)


def normalised_error(S, ref, cov_diag_a, cov_diag_b):
    return float(np.max(np.abs(S - ref) / np.sqrt(np.outer(cov_diag_a, cov_diag_b))))


def make_engine(oracle, windows, n, slides=0, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    eng = Engine(EngineOpts(windows=windows, capacity=n + 64, **kw))
    for w in range(windows):
        seq = synth.make_sequence(seed=40 + w, n_kf=n + slides + 1)
        prob = helpers.build_problem(oracle, seq, perturb=0.01)
        helpers.load_engine(eng, w, prob, lo=0, hi=n)
    eng.iterate(3)
    for _ in range(slides):
        eng.slide(marginalize=True)
        eng.iterate(3)
    return eng


EPS = np.finfo(np.float64).eps


def factor_inverse(P):
    """(L L^T)^-1 of the device's own factor, L rebuilt from vf_engine_read_panels (rows [k+1][k+2 pose][k+3 pose], L_kk^-T)"""
    n = P.shape[0]
    L = np.zeros((15 * n, 15 * n))
    for k in range(n):
        L[15 * k:15 * k + 15, 15 * k:15 * k + 15] = np.linalg.inv(P[k, 28:43, :15].T)
        for r in range(27):
            kk, a = (k + 1, r) if r < 15 else ((k + 2, r - 15) if r < 21 else (k + 3, r - 21))
            if kk < n:
                L[15 * kk + a, 15 * k:15 * k + 15] = P[k, r, :15]
    Li = np.linalg.inv(L)
    return Li.T @ Li


def block_error(cov, cross, S):
    n = cov.shape[0]
    dg = np.diag(S)
    err = 0.0
    for k in range(n):
        dk = dg[15 * k:15 * k + 15]
        err = max(err, normalised_error(cov[k], S[15 * k:15 * k + 15, 15 * k:15 * k + 15], dk, dk))
        if k + 1 < n:
            dk1 = dg[15 * (k + 1):15 * (k + 1) + 15]
            err = max(err, normalised_error(cross[k], S[15 * (k + 1):15 * (k + 1) + 15, 15 * k:15 * k + 15], dk1, dk))
        else:
            assert np.all(cross[k] == 0)
    return err


def check_against_dense(eng, ranges):
    """Every Sigma_kk and Sigma_{k+1,k} of each window (a) against the exact inverse of the device's factor, bar 1e-8 on entries
    normalised by sqrt(Sigma_ii Sigma_jj): what selected inversion itself adds; (b) against np.linalg.inv of the dense H
    (vf_engine_read_normal, lambda 0).  (b) cannot meet 1e-8 here: the windows' H have a condition number of ~1e12 even after
    diagonal scaling (prior information 1e14 beside between-factor information 1e1), so any two float64 inverses of it -- numpy's
    own Cholesky-based and LU-based ones included -- differ by up to cond * eps ~ 1e-4 normalised (measured 1.7e-5 between those
    two).  Its bar is that number, printed with cond(H)."""
    for w, (lo, hi) in enumerate(ranges):
        n = hi - lo
        Hb, _ = eng.read_normal(w, lo, n)
        Sref, cs, c = dense_inverse(dense_H(Hb))
        cov, cross = eng.read_marginals(w, lo, n, cross=True)
        ea = block_error(cov, cross, factor_inverse(eng.read_panels(w, lo, n)))
        eb = block_error(cov, cross, Sref)
        print(f"window {w} [{lo},{hi}): vs the device factor's inverse {ea:.3e}; vs the dense inverse of H {eb:.3e}, "
              f"cond(H) {c:.3e}, diagonally scaled {cs:.3e} (bar cond * eps = {cs * EPS:.3e})")
        assert ea < 1e-8, (w, ea)
        assert eb < cs * EPS, (w, eb, cs)


def test_engine_against_dense_inverse(oracle):
    """4 windows x 200 keyframes, bandwidth-3 between factors, a marginal prior from 3 marginalised slides"""
    eng = make_engine(oracle, 4, 200, slides=3)
    eng.marginals()
    check_against_dense(eng, [(3, 203)] * 4)
    # the panels read back afterwards are the undamped ones: their L_kk^-T reproduces Sigma of the last keyframe
    p = eng.read_panels(0, 202, 1)[0]
    U = p[28:43, :15]
    cov = eng.read_marginals(0, 202, 1)[0]
    assert np.allclose(U @ U.T, cov, rtol=1e-10, atol=0)
    eng.close()


def test_one_window_partitioned_and_assembling_batch_agree(oracle):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    n = 160
    seq = synth.make_sequence(seed=77, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.01)
    one = Engine(EngineOpts(windows=1, capacity=n + 64, chunks=0))
    helpers.load_engine(one, 0, prob)
    assert one.solve_form() == "partitioned"
    big = Engine(EngineOpts(windows=768, capacity=n + 64))
    for w in (0, 767):
        helpers.load_engine(big, w, prob)
    assert big.solve_form() == "assembling"
    # the same states in both (the solves of the two forms round differently)
    one.iterate(3)
    st = one.get_states(0, 0, n)
    for w in (0, 767):
        big.set_states(w, 0, st)
    for e in (one, big):
        e.marginals()
    a = one.read_marginals(0, 0, n, cross=True)
    _, cs, c = dense_inverse(dense_H(one.read_normal(0, 0, n)[0]))
    for w in (0, 767):
        b = big.read_marginals(w, 0, n, cross=True)
        d = np.sqrt(np.einsum("kii->ki", a[0]))
        e0 = np.max(np.abs(a[0] - b[0]) / np.einsum("ki,kj->kij", d, d))
        e1 = np.max(np.abs(a[1][:-1] - b[1][:-1]) / np.einsum("ki,kj->kij", d[1:], d[:-1]))
        print(f"one-window vs 768-window engine, window {w}: normalised difference {e0:.3e} / cross {e1:.3e}; "
              f"cond(H) {c:.3e}, diagonally scaled {cs:.3e}")
        # two elimination orders of the same H (plain sweep from H, assembling sweep from the J stream): rounding amplified by cond(H)
        assert 0 <= e0 < cs * EPS and e1 < cs * EPS
    one.close()
    big.close()


def _lm_snapshot(e, n):
    return e.get_states(0, 0, n), e.read_lm(0), e.read_delta(0, 0, n)


@pytest.mark.parametrize("kind", ["async", "reference_compat"])
def test_marginals_leave_the_lm_state_alone(oracle, kind):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    n = 120
    seq = synth.make_sequence(seed=91, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.01)
    out = []
    for with_marginals in (False, True):
        e = Engine(EngineOpts(windows=1, capacity=n + 64))
        helpers.load_engine(e, 0, prob)
        if kind == "async":
            e.set_async(True)
        step = (lambda: e.iterate(3)) if kind == "async" else (lambda: e.isam_step(1e-4))
        step()
        if with_marginals:
            e.marginals()
            if kind == "reference_compat":
                # Sigma is taken at theta: the states get_states returns, the points H was assembled at
                check_against_dense(e, [(0, n)])
        step()
        s, lm, d = _lm_snapshot(e, n)
        out.append((s, lm, d, e.get_estimate(0, 0, n) if kind == "reference_compat" else None))
        e.close()
    (s0, lm0, d0, x0), (s1, lm1, d1, x1) = out
    assert np.array_equal(s0, s1)
    assert lm0 == lm1
    assert np.array_equal(d0, d1)
    if x0 is not None:
        assert np.array_equal(x0, x1)


def _feed_handle(gm, seq, n, far=None, cb_store=None):
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


def test_handle_getter_and_callback(oracle):
    from vil_sensor_fusion_amd._lib import VilFusionError
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n, lag = 240, 200
    seq = synth.make_sequence(seed=5, n_kf=n)
    gm = GraphManager(capacity=n + 64, iterations=4, lag=lag)
    with pytest.raises(VilFusionError) as ex:
        gm.marginalCovariance(0)
    assert ex.value.code == -1                               # before the first solve
    got = []
    gm.addCovarianceCallback(lambda t, q, p, v, b, cov: got.append((t, cov.copy())))
    _feed_handle(gm, seq, n)
    assert len(got) == n - 1
    last = n - 1
    S = gm.marginalCovariance(last)
    assert np.array_equal(S, got[-1][1])                     # the callback's matrix is the getter's
    assert np.array_equal(S, S.T)
    assert np.all(np.linalg.eigvalsh(S) > 0)
    assert np.array_equal(gm.marginalCovariance(last), S)   # cached
    oldest = last - lag + 1
    gm.marginalCovariance(oldest)
    for key in (oldest - 1, last + 1):
        with pytest.raises(VilFusionError) as ex:
            gm.marginalCovariance(key)
        assert ex.value.code == -2                           # marginalised / not solved yet
    gm.close()


def test_handle_equals_engine_dense_inverse(oracle):
    """a whole-history handle (lag 0) against an engine that holds what the handle's engine held -- the IMU factors the handle
    preintegrated (vf_get_imu_factor), the between factors it was given, the anchor prior, the states it solved for -- and the
    dense inverse of that engine's H"""
    from vil_sensor_fusion_amd import Engine, EngineOpts
    from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 80
    seq = synth.make_sequence(seed=12, n_kf=n)
    gm = GraphManager(capacity=128, iterations=4, lag=0)
    _feed_handle(gm, seq, n)
    S = np.stack([gm.marginalCovariance(k) for k in range(n)])
    st = gm.trajectory(0, n)
    imu = np.stack([gm.imuFactor(k) for k in range(1, n)])
    gm.close()
    m = seq.btw_a >= 1
    eng = Engine(EngineOpts(windows=1, capacity=128))
    eng.set_states(0, 0, st)
    eng.set_imu(0, 1, imu)
    eng.set_between(0, seq.btw_a[m], seq.btw_b[m], synth.between_records(seq)[m])
    anchor = np.zeros(16)
    anchor[0] = 1.0
    eng.set_prior(0, 0, synth.prior_record(anchor, REFERENCE_PRIOR_SIGMAS))
    eng.set_range(0, 0, n)
    eng.marginals()
    check_against_dense(eng, [(0, n)])
    E = eng.read_marginals(0, 0, n)
    _, cs, c = dense_inverse(dense_H(eng.read_normal(0, 0, n)[0]))
    d = np.sqrt(np.einsum("kii->ki", E))
    diff = np.max(np.abs(S - E) / np.einsum("ki,kj->kij", d, d))
    print(f"handle vs engine on the handle's factors and states: max normalised difference {diff:.3e}; diagonally scaled cond(H) {cs:.3e}")
    assert diff < cs * EPS
    eng.close()


def test_handle_with_a_far_factor_refuses(oracle):
    from vil_sensor_fusion_amd._lib import VilFusionError
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 40
    seq = synth.make_sequence(seed=8, n_kf=n)
    gm = GraphManager(capacity=128, iterations=3, lag=0)
    got = []
    gm.addCovarianceCallback(lambda t, q, p, v, b, cov: got.append(cov.copy()))
    _feed_handle(gm, seq, n, far=(10, 30))
    with pytest.raises(VilFusionError) as ex:
        gm.marginalCovariance(n - 1)
    assert ex.value.code == -1 and "far" in str(ex.value)
    assert np.all(np.isnan(got[-1])) and np.all(np.isfinite(got[0]))
    gm.close()
