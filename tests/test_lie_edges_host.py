"""The CPU oracle's SO(3) / SE(3) maps and factor restatements against the mpmath reference (tests/mp_lie.py) at the
rotation angles where the series / closed-form switches sit and where the closed forms lose digits (mp_lie.EDGE_ANGLES),
with translations up to 100 m so that the E W^2 t term of Pose3's Logmap matters.

Bars: maps to a few ulps of the result's scale (max |entry|), each stated below; factor residuals and Jacobians to
1e-12 * max|block|, the bar the GPU parity tests hold the device to (tests/test_gpu_parity.py).  The oracle judges the
device, so it has to be right where they share a formula: before the half-angle form of E (vf_oracle.c coef_E) the
near-pi cases failed here by 1e-10 .. 1e-8."""
import numpy as np
import pytest

from tests import mp_lie as M

EPS = np.finfo(np.float64).eps
TOL = 1e-12
ANGLES = M.EDGE_ANGLES


def scaled(a, ref):
    """max |a - ref| in units of max |ref| (ulps of the result's scale when divided by EPS)"""
    return float(np.abs(np.asarray(a) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300))


def rand_q(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def rot(w):
    return [M.vec(r) for r in np.asarray(w).reshape(3, 3)]


@pytest.mark.parametrize("ang", ANGLES)
def test_so3_maps(oracle, ang):
    rng = np.random.default_rng(int(ang * 1e6) % 2**31 + 1)
    w = M.axis(rng) * ang
    wm = M.vec(w)
    R = oracle.so3_exp(w)
    # Exp: entries are O(1); sin / cos of theta and a 2-term sum: 4 ulps
    assert scaled(R, M.to_np(M.so3_exp_w(wm))) <= 4 * EPS
    # Log of the double matrix the oracle returned (not of the nominal w): Shepperd + atan2, 8 ulps of theta
    assert scaled(oracle.so3_log(R), M.to_np(M.so3_log_R(rot(R)))) <= 8 * EPS
    # J_r and J_r^{-1}: I + 2 terms whose coefficients come from x = |w|^2 (one rounding there): 8 ulps of max |J|
    assert scaled(oracle.so3_jr(w), M.to_np(M.so3_jr_w(wm))) <= 8 * EPS
    assert scaled(oracle.so3_jr_inv(w), M.to_np(M.so3_jr_inv_w(wm))) <= 8 * EPS


@pytest.mark.parametrize("ang", ANGLES)
def test_se3_maps(oracle, ang):
    rng = np.random.default_rng(int(ang * 1e6) % 2**31 + 2)
    w = M.axis(rng) * ang
    v = rng.normal(size=3) * 40.0          # |v| up to ~100 m
    R, t = oracle.se3_exp(np.concatenate([w, v]))
    Rm, tm = M.se3_exp_w(M.vec(w), M.vec(v))
    # Exp: t = J_l(w) v, 3 terms of |v| scale: 8 ulps of max |t|
    assert scaled(R, M.to_np(Rm)) <= 4 * EPS
    assert scaled(t, M.to_np(tm)) <= 8 * EPS
    # Log of the doubles (R, t) the oracle returned: u = (I - W/2 + E W^2) t, terms up to theta^2 |t| ~ 10 |u|: 16 ulps
    xi = oracle.se3_log(R, t)
    wr, ur = M.se3_log_Rt(rot(R), M.vec(t))
    assert scaled(xi[:3], M.to_np(wr)) <= 8 * EPS
    assert scaled(xi[3:], M.to_np(ur)) <= 16 * EPS, (scaled(xi[3:], M.to_np(ur)) / EPS)
    # LogmapDerivative at the double xi: blocks J_r^{-1}(w) and Q2 = D J_r^{-1}(w)[u] (entries up to |u| theta^2 / 12);
    # Q2 sums 4 products whose terms reach theta |u|: 32 ulps of max |J|
    Jm = M.to_np(M.se3_jr_inv_xi(M.vec(xi[:3]), M.vec(xi[3:])))
    err = scaled(oracle.se3_jr_inv(xi), Jm)
    assert err <= 32 * EPS, err / EPS


def between_case(oracle, rng, ang):
    """(rec, xa, xb): the error pose measured^-1 * (xa^-1 xb) is Exp([ang * axis, u]) with |u| up to ~100 m"""
    A = rng.normal(size=(6, 6))
    cov = A @ A.T * 0.05 + np.eye(6) * 0.01
    qm = rand_q(rng)
    tm = rng.normal(size=3) * 3.0
    rec = np.concatenate([qm, tm, oracle.sqrt_info_upper(cov)])
    xa = np.concatenate([rand_q(rng), rng.normal(size=3) * 50, rng.normal(size=9)])
    Ra, Rm = oracle.quat_to_rot(xa[:4]), oracle.quat_to_rot(qm)
    Re, te = oracle.se3_exp(np.concatenate([M.axis(rng) * ang, rng.normal(size=3) * 40.0]))
    xb = np.concatenate([oracle.rot_to_quat(Ra @ Rm @ Re), xa[4:7] + Ra @ (tm + Rm @ te), rng.normal(size=9)])
    return rec, xa, xb


def prior_case(oracle, rng, ang):
    mean = np.concatenate([rand_q(rng), rng.normal(size=3) * 50, rng.normal(size=3), rng.normal(size=6) * 0.05])
    sig = np.array([1e-2] * 3 + [5e-2] * 3 + [1e-1] * 3 + [1e-3] * 6)
    d = np.concatenate([M.axis(rng) * ang, rng.normal(size=3) * 40.0, rng.normal(size=9) * 0.1])
    return np.concatenate([mean, sig]), oracle.retract(mean, d)


def pim_record(oracle, rng, theta, n=40, dt=0.0025, bhat=None):
    """an IMU record whose preintegrated rotation is ~theta: a constant turn (theta grows linearly for a fixed axis) plus noise"""
    bhat = np.zeros(6) if bhat is None else bhat
    ax = M.axis(rng)
    prm = oracle.carla_imu_params()
    p = oracle.pim_new(bhat)
    for _ in range(n):
        gyr = ax * theta / (n * dt) + bhat[3:] + rng.normal(size=3) * 1e-3
        acc = np.array([0.3, -0.2, 9.81]) + bhat[:3] + rng.normal(size=3) * 0.5
        oracle.pim_integrate(p, prm, acc, gyr, dt)
    return oracle.pim_to_record(p)


def imu_case(oracle, rng, theta_pim, ang):
    """(rec, xi, xj): preintegrated rotation ~theta_pim, bias of xi 0.1 rad/s (gyro) off bhat, rotation residual ~ang"""
    bhat = np.array([0.02, -0.01, 0.03, 0.01, -0.02, 0.005])
    rec = pim_record(oracle, rng, theta_pim, bhat=bhat)
    g = np.array([0.0, 0.0, -9.81])
    xi = np.concatenate([rand_q(rng), rng.normal(size=3) * 50, rng.normal(size=3) * 5, bhat + [0.01, 0.02, -0.01, 0.1, -0.05, 0.08]])
    xj = oracle.predict(rec, g, xi)
    # the residual's rotation is Log(Rj^T Rpred): rotate xj by Exp(-ang * axis) on the right
    xj = oracle.retract(xj, np.concatenate([-M.axis(rng) * ang, rng.normal(size=3), rng.normal(size=3) * 0.5,
                                            rng.normal(size=6) * 0.01]))
    return rec, g, xi, xj


@pytest.mark.parametrize("ang", ANGLES[1:])
def test_between_factor(oracle, ang):
    rng = np.random.default_rng(100 + ANGLES.index(ang))
    rec, xa, xb = between_case(oracle, rng, ang)
    r, Ja, Jb = oracle.between_factor(rec, xa, xb)
    rm, Jam, Jbm = M.between_factor(rec, xa, xb)
    errs = scaled(r, rm), scaled(Ja, Jam), scaled(Jb, Jbm)
    print(f"between {ang:.10g}: r {errs[0]:.1e} Ja {errs[1]:.1e} Jb {errs[2]:.1e}")
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("ang", ANGLES[1:])
def test_prior_factor(oracle, ang):
    rng = np.random.default_rng(200 + ANGLES.index(ang))
    rec, x = prior_case(oracle, rng, ang)
    r, J = oracle.prior_factor(rec, x)
    rm, Jm = M.prior_factor(rec, x)
    errs = scaled(r[:6], rm[:6]), scaled(J[:6, :6], Jm[:6, :6]), scaled(r[6:], rm[6:]), scaled(J[6:], Jm[6:])
    print(f"prior {ang:.10g}: r {errs[0]:.1e} J {errs[1]:.1e}")
    assert max(errs) <= TOL, errs


IMU_CASES = [(0.02, a) for a in ANGLES[1:]] + [(t, 0.3) for t in (0.4999999, 0.5000001, 1.3, 2.9, np.pi - 1e-6)] + \
    [(2.0, np.pi - 1e-6), (np.pi - 1e-3, np.pi - 1e-8)]


@pytest.mark.parametrize("theta_pim,ang", IMU_CASES)
def test_imu_factor(oracle, theta_pim, ang):
    rng = np.random.default_rng(int(theta_pim * 1000) * 7 + IMU_CASES.index((theta_pim, ang)))
    rec, g, xi, xj = imu_case(oracle, rng, theta_pim, ang)
    r, J = oracle.imu_factor(rec, g, xi, xj)
    rm, Jm = M.imu_factor(rec, g, xi, xj)
    errs = scaled(r, rm), scaled(J, Jm)
    print(f"imu theta~{theta_pim:.10g} r_theta~{ang:.10g}: |r_theta| {np.linalg.norm(oracle.imu_factor(rec, g, xi, xj, False)[0][:3]):.10g} "
          f"r {errs[0]:.1e} J {errs[1]:.1e}")
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("ang", ANGLES)
def test_retract(oracle, ang):
    rng = np.random.default_rng(300 + ANGLES.index(ang))
    x = np.concatenate([rand_q(rng), rng.normal(size=3) * 50, rng.normal(size=9)])
    d = np.concatenate([M.axis(rng) * ang, rng.normal(size=3) * 40.0, rng.normal(size=9)])
    out = oracle.retract(x, d)
    ref = M.retract(x, d).to_np()
    if np.dot(out[:4], ref[:4]) < 0:   # q and -q are one rotation: rot_to_quat picks w >= 0 of rounded matrices
        ref[:4] = -ref[:4]
    # quaternion: product of two rotation matrices and Shepperd, 8 ulps; translation t + R J_l(w) v: 16 ulps of max |t|
    assert scaled(out[:4], ref[:4]) <= 8 * EPS
    assert scaled(out[4:7], ref[4:7]) <= 16 * EPS
    np.testing.assert_array_equal(out[7:], x[7:] + d[6:])


@pytest.mark.parametrize("theta_pim", [0.0, 0.4999999, 0.5000001, 1.3, 2.0, 2.9, 3.0])
def test_predict(oracle, theta_pim):
    rng = np.random.default_rng(400 + int(theta_pim * 100))
    rec = pim_record(oracle, rng, theta_pim, bhat=np.array([0.02, -0.01, 0.03, 0.01, -0.02, 0.005]))
    g = np.array([0.0, 0.0, -9.81])
    xi = np.concatenate([rand_q(rng), rng.normal(size=3) * 50, rng.normal(size=3) * 5, rng.normal(size=6) * 0.05])
    out = oracle.predict(rec, g, xi)
    ref = M.predict(rec, g, xi)
    if np.dot(out[:4], ref[:4]) < 0:
        ref[:4] = -ref[:4]
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"predict theta~{theta_pim}: {err:.1e}")
    assert err <= TOL     # the bar of test_gpu_parity.test_predict_parity

