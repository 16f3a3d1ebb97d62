"""References of the innovation gate (vf_engine_gate_tail, kernels/kgate.inc), tests only.

For the last keyframe i of a solved window (state x_i, marginal Sigma_ii), the raw IMU steps that follow it, a keyframe a in {i, i-1}
(state x_a, pose marginal Sigma_aa^pp, and Sigma_{i,a} = Cov(x_i, x_a): Sigma_ii itself when a = i, the cross block Sigma_{i,i-1} with
row = dof of i when a = i-1) and a BetweenFactor<Pose3> record from a to the keyframe j the steps lead to:

    x_j      = predict(record of the steps, x_i)                               (tests/propagate_ref.py)
    d_j      = G d_i + B^-1 n,  G = -B^-1 A,  n ~ N(0, P)                      A, B: unwhitened IMU Jacobians at zero residual
    Sjj      = (G Sigma_ii G^T + B^-1 P B^-T)[0:6, 0:6]
    C        = (G Sigma_{i,a})[0:6, 0:6]                                       Cov(pose_j, pose_a)
    r, Ja, Jb  whitened between factor at (x_a, x_j); xi its unwhitened residual [rot, trans]
    S        = I + Ja Saa Ja^T + Ja C^T Jb^T + Jb C Ja^T + Jb Sjj Jb^T
    nis      = r^T S^-1 r,   nis_measurement = r^T r

Without steps x_j = x_i, G = I, P = 0.  Tangent order of vf_engine_read_marginals.

  * `gate_mp`: extended precision.  P from tests/mp_pim.preintegrate_mp; the state, A, B from tests/mp_lie.predict /
    mp_lie.imu_factor(whiten=False); r, Ja, Jb, xi from mp_lie.between_factor; the products, B^-1 and S^-1 r in mpmath, from the
    float64 blocks taken as exact input.  Also returns `gp_rows`: max |(-B^-1 A)[0:6, :] - A[0:6, :]|, the claim the kernel rests on
    (B touches the velocity rows only, so the pose rows of G are the first six rows of A).
  * `gate_f64`: the same statement in numpy on the CPU oracle, every product accumulated term by term (propagate_ref._mm), the
    6 x 6 solve by a Cholesky factorisation written out here (no LAPACK: the same bits on every host).
  * `measurement`: a record whose measured pose is the predicted relative pose moved by a tangent vector."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import mp_lie, mp_pim
from tests.propagate_ref import COLS_I, COLS_J, GRAVITY, _mm, _record


def _mpm(a):
    return mp.matrix(np.asarray(a, dtype=np.float64).tolist())


def gate_mp(steps, cov, x_i, x_a, sigma_ii, sigma_ia, sigma_aa_pp, rec28, gravity=GRAVITY):
    """dict nis, nis_measurement (float64, rounded once), xi (6,), state (16,), S (6, 6), gp_rows"""
    x_i, x_a = np.asarray(x_i, dtype=np.float64), np.asarray(x_a, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1, 7)
    Sii, Sia, Saa = _mpm(sigma_ii), _mpm(sigma_ia), _mpm(np.asarray(sigma_aa_pp)[:6, :6])
    if steps.shape[0] == 0:
        x_j, G, N, gp_rows = x_i.copy(), mp.eye(15), mp.zeros(15, 15), 0.0
    else:
        bhat = x_i[10:16]
        r = mp_pim.preintegrate_mp(steps, bhat, cov)
        rec = _record(float(r["dt"]), mp_pim._f64(r["mean"]), bhat, mp_pim._f64(r["H"]))
        x_j = mp_lie.predict(rec, gravity, x_i)
        _, J = mp_lie.imu_factor(rec, gravity, x_i, x_j, whiten=False)
        A, B = _mpm(J[:, COLS_I]), _mpm(J[:, COLS_J])
        Bi = mp.inverse(B)
        G = -Bi * A
        N = Bi * mp.matrix(r["P"].tolist()) * Bi.T
        gp_rows = float(max(abs(G[a, c] - A[a, c]) for a in range(6) for c in range(15)))
    Gp = G[0:6, :]
    Sjj = (Gp * Sii * Gp.T + N[0:6, 0:6])
    Cx = (Gp * Sia)[:, 0:6]
    rw, Ja, Jb = mp_lie.between_factor(rec28, x_a, x_j)
    xi = mp_lie.between_factor(rec28, x_a, x_j, whiten=False)[0]
    rw, Ja, Jb = _mpm(rw.reshape(6, 1)), _mpm(Ja), _mpm(Jb)
    S = mp.eye(6) + Ja * Saa * Ja.T + Ja * Cx.T * Jb.T + Jb * Cx * Ja.T + Jb * Sjj * Jb.T
    S = (S + S.T) / 2
    y = mp.lu_solve(S, rw)
    nis = (rw.T * y)[0, 0]
    return dict(nis=float(nis), nis_measurement=float((rw.T * rw)[0, 0]), xi=xi, state=x_j, gp_rows=gp_rows,
                S=np.array([[float(S[a, c]) for c in range(6)] for a in range(6)]))


def _chol_solve_quadratic(S, r):
    """r^T S^-1 r by S = L L^T, y = L^-1 r, in plain float64 loops"""
    L, y = np.zeros((6, 6)), np.zeros(6)
    for c in range(6):
        d = S[c, c] - sum(L[c, k] * L[c, k] for k in range(c))
        if not d > 0.0:
            return float("nan")
        L[c, c] = np.sqrt(d)
        for i in range(c + 1, 6):
            L[i, c] = (S[i, c] - sum(L[i, k] * L[c, k] for k in range(c))) / L[c, c]
        y[c] = (r[c] - sum(L[c, k] * y[k] for k in range(c))) / L[c, c]
    return float(sum(v * v for v in y))


def predict_f64(oracle, steps, cov, x_i, gravity=GRAVITY):
    """(x_j, A, B, P) of the steps on the CPU oracle; without steps (x_i, I, -I, 0)"""
    x_i = np.asarray(x_i, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1, 7)
    if steps.shape[0] == 0:
        return x_i.copy(), np.eye(15), -np.eye(15), np.zeros((15, 15))
    prm = oracle.make_imu_params(cov["acc"], cov["gyro"], cov["integration"], cov["bias_acc"], cov["bias_omega"], cov["bias_acc_omega_int"])
    p = oracle.pim_new(x_i[10:16])
    for s in steps:
        oracle.pim_integrate(p, prm, s[1:4], s[4:7], s[0])
    f = oracle.pim_fields(p)
    rec = _record(f["dt"], f["d"], f["bhat"], f["H"])
    x_j = oracle.predict(rec, gravity, x_i)
    _, J = oracle.imu_factor(rec, gravity, x_i, x_j, whiten=False)
    return x_j, J[:, COLS_I], J[:, COLS_J], f["cov"]


def gate_f64(oracle, steps, cov, x_i, x_a, sigma_ii, sigma_ia, sigma_aa_pp, rec28, gravity=GRAVITY):
    """dict nis, nis_measurement, xi, state, S in float64 from the CPU oracle"""
    x_j, A, B, P = predict_f64(oracle, steps, cov, x_i, gravity)
    Bi = np.linalg.inv(B)
    Gp = -_mm(Bi, A)[:6]
    N = _mm(_mm(Bi, P), Bi.T)[:6, :6]
    Sjj = _mm(_mm(Gp, sigma_ii), Gp.T) + N
    Cx = _mm(Gp, sigma_ia)[:, :6]
    Saa = np.asarray(sigma_aa_pp, dtype=np.float64)[:6, :6]
    r, Ja, Jb = oracle.between_factor(rec28, x_a, x_j)
    xi = oracle.between_factor(rec28, x_a, x_j, whiten=False)[0]
    S = np.eye(6) + _mm(_mm(Ja, Saa), Ja.T) + _mm(_mm(Ja, Cx.T), Jb.T) + _mm(_mm(Jb, Cx), Ja.T) + _mm(_mm(Jb, Sjj), Jb.T)
    S = 0.5 * (S + S.T)
    return dict(nis=_chol_solve_quadratic(S, r), nis_measurement=float(sum(v * v for v in r)), xi=xi, state=x_j, S=S)


# a covariance of an odometry increment that is not diagonal: sigmas of 2 mrad and 2 cm, correlations up to 0.4
def cov36():
    s = np.array([2e-3, 2.5e-3, 1.5e-3, 2e-2, 1.5e-2, 2.5e-2])
    c = np.eye(6)
    for (a, b), v in {(0, 1): 0.3, (0, 4): -0.2, (2, 3): 0.4, (3, 5): 0.25, (1, 5): -0.1}.items():
        c[a, b] = c[b, a] = v
    return c * np.outer(s, s)


CONSISTENT = 0.3 * np.array([0.5, -0.4, 0.3, -0.45, 0.35, 0.4])     # in sigmas (a vector of length 1 x 0.3), through chol(cov36)
GROSS = np.array([0.3 * 0.6, 0.3 * 0.0, 0.3 * 0.8, 0.6, -0.64, 0.48])    # 0.3 rad and 1 m


def measurement(oracle, x_a, x_j, cov, kind):
    """the 28-double record of a between factor a -> j measuring T_a^-1 T_j Exp(d): d = chol(cov) CONSISTENT (0.3 sigma) or GROSS"""
    d = np.linalg.cholesky(cov) @ CONSISTENT if kind == "consistent" else GROSS
    Ra, Rj = oracle.quat_to_rot(x_a[:4]), oracle.quat_to_rot(x_j[:4])
    Rh, th = Ra.T @ Rj, Ra.T @ (x_j[4:7] - x_a[4:7])
    Rd, td = oracle.se3_exp(d)
    rec = np.zeros(28)
    rec[0:4] = oracle.rot_to_quat(Rh @ Rd)
    rec[4:7] = th + Rh @ td
    rec[7:28] = oracle.sqrt_info_upper(cov)
    return rec
