"""References of the IMU-rate prediction (vf_engine_propagate_tail, kernels/kprop.inc), tests only.

For a keyframe i with state x_i (its bias is the bias estimate the samples are integrated with), marginal covariance Sigma_ii
and the raw IMU steps that follow it:

    state   x_j = predict(record of the steps, x_i)                              (PreintegrationBase::predict)
    Sigma+  = B^-1 (A Sigma_ii A^T + P) B^-T

P the 15 x 15 preintegrated covariance of the steps, A and B the UNWHITENED Jacobians of the combined-IMU factor's residual with
respect to the 15 dof of keyframe i and of keyframe j, evaluated at x_j = the prediction (zero residual).  Tangent order of
vf_engine_read_marginals: [omega, v] of Pose3, velocity, bias acc, bias gyro -- the order of the factor's residual and of P.
Without steps the result is x_i and Sigma_ii themselves.

  * `propagate_mp`: the extended-precision reference.  P from tests/mp_pim.preintegrate_mp; A, B and the state from
    tests/mp_lie.imu_factor(whiten=False) / mp_lie.predict on the record of that preintegration (their central differences in
    mpmath, not the closed forms the kernel uses); Sigma+ evaluated in mpmath, B inverted there, from the float64 Sigma_ii taken
    as exact input.
  * `propagate_f64`: the same statement in numpy on the CPU oracle: oracle.pim_* for the record and P, oracle.predict,
    oracle.imu_factor(whiten=False).
  * `error`: max |S - ref| / sqrt(ref_ii ref_jj)."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import mp_lie, mp_pim

GRAVITY = np.array([0.0, 0.0, -9.81])
COLS_I = list(range(0, 9)) + list(range(18, 24))      # columns of the 15 x 30 Jacobian: [pose_i, vel_i, pose_j, vel_j, bias_i, bias_j]
COLS_J = list(range(9, 18)) + list(range(24, 30))


def _record(dt, mean, bhat, H):
    """the 190-double record without a noise model (unwhitened factors never read it)"""
    return np.concatenate([[dt], mean, bhat, np.asarray(H).ravel(), np.zeros(120)])


def propagate_mp(steps, cov, x_i, sigma_ii, gravity=GRAVITY):
    """dict state (16,), cov (15, 15), P (15, 15) as float64 (rounded once from mpmath) and cov_mp, the mpf matrix"""
    x_i = np.asarray(x_i, dtype=np.float64)
    sigma_ii = np.asarray(sigma_ii, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1, 7)
    if steps.shape[0] == 0:
        return dict(state=x_i.copy(), cov=sigma_ii.copy(), P=np.zeros((15, 15)), cov_mp=mp.matrix(sigma_ii.tolist()))
    bhat = x_i[10:16]
    r = mp_pim.preintegrate_mp(steps, bhat, cov)
    rec = _record(float(r["dt"]), mp_pim._f64(r["mean"]), bhat, mp_pim._f64(r["H"]))
    x_j = mp_lie.predict(rec, gravity, x_i)
    _, J = mp_lie.imu_factor(rec, gravity, x_i, x_j, whiten=False)
    A, B = mp.matrix(J[:, COLS_I].tolist()), mp.matrix(J[:, COLS_J].tolist())
    P = mp.matrix(r["P"].tolist())
    Bi = mp.inverse(B)
    S = Bi * (A * mp.matrix(sigma_ii.tolist()) * A.T + P) * Bi.T
    return dict(state=x_j, cov=np.array([[float(S[a, c]) for c in range(15)] for a in range(15)]), P=mp_pim._f64(r["P"]), cov_mp=S)


def _mm(A, B):
    """A B in float64 with every entry accumulated term by term in index order (no BLAS: the same bits on every host)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = np.zeros((A.shape[0], B.shape[1]))
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            acc = 0.0
            for l in range(A.shape[1]):
                acc += float(A[i, l]) * float(B[l, j])
            out[i, j] = acc
    return out


def propagate_f64(oracle, steps, cov, x_i, sigma_ii, gravity=GRAVITY):
    """dict state, cov, P in float64 from the CPU oracle"""
    x_i = np.asarray(x_i, dtype=np.float64)
    sigma_ii = np.asarray(sigma_ii, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1, 7)
    if steps.shape[0] == 0:
        return dict(state=x_i.copy(), cov=sigma_ii.copy(), P=np.zeros((15, 15)))
    prm = oracle.make_imu_params(cov["acc"], cov["gyro"], cov["integration"], cov["bias_acc"], cov["bias_omega"], cov["bias_acc_omega_int"])
    p = oracle.pim_new(x_i[10:16])
    for s in steps:
        oracle.pim_integrate(p, prm, s[1:4], s[4:7], s[0])
    f = oracle.pim_fields(p)
    rec = _record(f["dt"], f["d"], f["bhat"], f["H"])
    x_j = oracle.predict(rec, gravity, x_i)
    _, J = oracle.imu_factor(rec, gravity, x_i, x_j, whiten=False)
    A, B = J[:, COLS_I], J[:, COLS_J]
    Bi = np.linalg.inv(B)
    S = _mm(_mm(Bi, _mm(_mm(A, sigma_ii), A.T) + f["cov"]), Bi.T)
    return dict(state=x_j, cov=0.5 * (S + S.T), P=f["cov"])


def error(S, ref):
    """max |S - ref| / sqrt(ref_ii ref_jj)"""
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(np.asarray(S) - ref) / np.outer(d, d)))


def state_error(x, ref):
    """max component difference of two states, the quaternions compared up to sign"""
    x, ref = np.asarray(x), np.asarray(ref)
    q = x[:4] if np.dot(x[:4], ref[:4]) >= 0 else -x[:4]
    return float(max(np.abs(q - ref[:4]).max(), np.abs(x[4:] - ref[4:]).max()))
