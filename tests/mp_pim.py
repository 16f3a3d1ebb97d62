"""High-precision reference of K0's whole record (tests only): dt_ij, the preintegrated mean, the 9 x 6 bias Jacobians H,
the 15 x 15 covariance P and its noise model R = chol_upper(P^-1), in mpmath at tests/mp_lie.DPS digits from the float64
inputs exactly as K0 and vfo_pim_integrate receive them.

Definitions: GTSAM 4.0.x, PreintegratedCombinedMeasurements::integrateMeasurement over TangentPreintegration::update.
Per step, with acc = a_meas - bhat_acc, om = w_meas - bhat_gyro and the one-step map of the tangent state (theta, p, v)

    theta' = theta + dt J_r^{-1}(theta) om,   p' = p + dt v + dt^2/2 Exp(theta) acc,   v' = v + dt Exp(theta) acc

  * A = d(theta', p', v') / d(theta, p, v).  Its theta columns are mpmath central differences of the map
    theta -> (J_r^{-1}(theta) om, Exp(theta) acc), NOT a restatement of the closed forms the code under test uses
    (so3_jr_apply_dtheta, a_nav_H_theta).  The p and v columns are linear and written out.
  * B = d(.)'/d acc = [0; dt^2/2 Exp(theta); dt Exp(theta)], C = d(.)'/d om = [dt J_r^{-1}(theta); 0; 0], and the bias
    Jacobians follow H <- A H - [B | C] (the chain rule through acc = a_meas - bhat_acc, om = w_meas - bhat_gyro).
  * F = [[A, Fb], [0, I]], whose bias blocks are those of 4.0.x's CombinedImuFactor: theta_H_biasOmega = -C.top,
    vel_H_biasAcc = -B.bottom.  There is no pos_H_biasAcc: GTSAM leaves it out too (the "TODO(frank)" beside that block
    in PreintegratedCombinedMeasurements::integrateMeasurement), so it is left out here on purpose.
  * P <- F P F^T + G Q G^T with the D_R_R, D_v_v blocks in the dt-multiplied form (gyro + int) dt J_r^{-1} J_r^{-T} and
    (acc + int) dt Exp(theta) Exp(theta)^T, algebraically GTSAM's (1/dt) tHb (.) tHb^T and (1/dt) vHb (.) vHb^T but defined
    at dt = 0, where the step is then an exact no-op; D_t_t = dt integration I, D_a_a = dt bias_acc I, D_g_g = dt bias_omega I.
  * R = chol_upper(P^-1): upper triangular, positive diagonal, R^T R = P^-1 (noiseModel::Gaussian::Covariance).  It is
    unique, so it can be compared entry by entry.

Self-check: H is also taken as the total derivative of the mean (mp_lie.preintegrate_mean_mp) with respect to bhat, by
central differences; the two agree to better than 1e-25 of max |H| or `reference` raises."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from tests import mp_lie as L
from tests import pim_cases

H_SELF_CHECK = 1e-25


def _mat(rows):
    return np.array(rows, dtype=object)


def _zeros(n, m):
    return _mat([[mp.mpf(0)] * m for _ in range(n)])


def _theta_cols(th, acc, om):
    """d(J_r^{-1}(theta) om)/d theta and d(Exp(theta) acc)/d theta, 3 x 3 each, by central differences in mpmath"""
    Dw, Da = _zeros(3, 3), _zeros(3, 3)
    for j in range(3):
        out = []
        for sg in (1, -1):
            t = list(th)
            t[j] += sg * L.H_FD
            out.append((L.mv(L.so3_jr_inv_w(t), om), L.mv(L.so3_exp_w(t), acc)))
        for i in range(3):
            Dw[i, j] = (out[0][0][i] - out[1][0][i]) / (2 * L.H_FD)
            Da[i, j] = (out[0][1][i] - out[1][1][i]) / (2 * L.H_FD)
    return Dw, Da


def preintegrate_mp(steps, bhat, cov):
    """the record in mpf: dict dt (mpf), mean (9), H (9 x 6), P (15 x 15) as object arrays of mpf"""
    b = L.vec(bhat)
    c = {k: L._m(v) for k, v in cov.items()}
    th, p, v = [mp.mpf(0)] * 3, [mp.mpf(0)] * 3, [mp.mpf(0)] * 3
    T = mp.mpf(0)
    H = _zeros(9, 6)
    P = _zeros(15, 15)
    for st in np.asarray(steps, dtype=np.float64):
        dt = L._m(st[0])
        dt22 = dt * dt / 2
        acc = L.vadd(L.vec(st[1:4]), b[0:3], -1)
        om = L.vadd(L.vec(st[4:7]), b[3:6], -1)
        Jinv = _mat(L.so3_jr_inv_w(th))
        Rt = _mat(L.so3_exp_w(th))
        Dw, Da = _theta_cols(th, acc, om)
        # F = [[A, Fb], [0, I]]; A = [[I + dt Dw, 0, 0], [dt^2/2 Da, I, dt I], [dt Da, 0, I]]
        Ath = _mat(L.eye(3)) + Dw * dt
        Bm, Cm = _zeros(9, 3), _zeros(9, 3)
        Bm[3:6], Bm[6:9] = Rt * dt22, Rt * dt
        Cm[0:3] = Jinv * dt

        def a_left(M):                                  # A M for a 9-row M
            DM = Da.dot(M[0:3])
            return np.concatenate([Ath.dot(M[0:3]), DM * dt22 + M[3:6] + M[6:9] * dt, DM * dt + M[6:9]])

        def fb_left(M):                                 # Fb M for a 6-row M (the bias rows)
            out = _zeros(9, M.shape[1])
            out[0:3] = -Cm[0:3].dot(M[3:6])             # theta_H_biasOmega = -C.top
            out[6:9] = -Bm[6:9].dot(M[0:3])             # vel_H_biasAcc = -B.bottom (no pos_H_biasAcc, as GTSAM)
            return out
        H = a_left(H) - np.concatenate([Bm, Cm], axis=1)
        X = a_left(P[0:9]) + fb_left(P[9:15])            # rows 0..8 of F P
        Pn = _zeros(15, 15)
        Pn[0:9, 0:9] = (a_left(X[:, 0:9].T) + fb_left(X[:, 9:15].T)).T
        Pn[0:9, 9:15] = X[:, 9:15]
        Pn[9:15, 0:9] = X[:, 9:15].T
        Pn[9:15, 9:15] = P[9:15, 9:15]
        gr, ar = c["gyro"] + c["bias_acc_omega_int"], c["acc"] + c["bias_acc_omega_int"]
        Pn[0:3, 0:3] += Jinv.dot(Jinv.T) * (gr * dt)
        Pn[6:9, 6:9] += Rt.dot(Rt.T) * (ar * dt)
        for i in range(3):
            Pn[3 + i, 3 + i] += dt * c["integration"]
            Pn[9 + i, 9 + i] += dt * c["bias_acc"]
            Pn[12 + i, 12 + i] += dt * c["bias_omega"]
        P = Pn
        wt, an = L.mv(Jinv.tolist(), om), L.mv(Rt.tolist(), acc)
        p = [p[i] + v[i] * dt + an[i] * dt22 for i in range(3)]
        v = [v[i] + an[i] * dt for i in range(3)]
        th = [th[i] + wt[i] * dt for i in range(3)]
        T += dt
    return dict(dt=T, mean=_mat(th + p + v), H=H, P=P)


def chol_upper_inv(P):
    """R upper with positive diagonal and R^T R = P^-1, in mpmath"""
    Pm = mp.matrix(P.tolist())
    Lc = mp.cholesky(mp.inverse(Pm))
    n = Pm.rows
    return _mat([[Lc[c, r] if c >= r else mp.mpf(0) for c in range(n)] for r in range(n)])


def bias_jacobian_fd(steps, bhat):
    """H as the total derivative d mean / d bhat, by central differences of mp_lie.preintegrate_mean_mp"""
    b = L.vec(bhat)
    J = _zeros(9, 6)
    for j in range(6):
        out = []
        for sg in (1, -1):
            bb = list(b)
            bb[j] += sg * L.H_FD
            out.append(L.preintegrate_mean_mp(steps, bb)[1])
        for i in range(9):
            J[i, j] = (out[0][i] - out[1][i]) / (2 * L.H_FD)
    return J


def _f64(A):
    return np.vectorize(float, otypes=[np.float64])(A)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the record of pim_cases.case(name): dict of float64 dt, mean (9), H (9 x 6), P (15 x 15), R (15 x 15, upper),
    rec (the 190-double record layout, R packed row-major), cond (of D P D, D = diag(P)^-1/2), h_self (the self-check's
    relative difference) and mp (the mpf values)"""
    _, steps, bhat, cov = pim_cases.case(name)
    r = preintegrate_mp(steps, bhat, cov)
    R = chol_upper_inv(r["P"])
    Hfd = bias_jacobian_fd(steps, bhat)
    hmax = max(abs(x) for x in r["H"].ravel())
    h_self = float(max(abs(x) for x in (r["H"] - Hfd).ravel()) / hmax)
    if not h_self < H_SELF_CHECK:
        raise AssertionError(f"{name}: the H recursion and d mean / d bhat differ by {h_self:.2e} of max |H|")
    P, Rf = _f64(r["P"]), _f64(R)
    d = 1.0 / np.sqrt(np.diag(P))
    rec = np.concatenate([[float(r["dt"])], _f64(r["mean"]), np.asarray(bhat, dtype=np.float64), _f64(r["H"]).ravel(),
                          Rf[np.triu_indices(15)]])
    return dict(dt=float(r["dt"]), mean=_f64(r["mean"]), H=_f64(r["H"]), P=P, R=Rf, rec=rec,
                cond=float(np.linalg.cond(d[:, None] * P * d[None, :])), h_self=h_self, mp=dict(r, R=R))


# ---------------------------------------------------------------- the measures the host and device tests share
EPS = float(np.finfo(np.float64).eps)


def errors(ref, dt, mean, H, R, P=None):
    """the per-case measures of a record against the reference: dt (relative), mean (relative to max |mean|), H (row-scaled),
    P (scaled by sqrt(P_ii P_jj) of the reference; None without P), whiten = |R P_ref R^T - I|, R (row-scaled entries)"""
    e = dict(dt=abs(dt - ref["dt"]) / ref["dt"] if ref["dt"] else abs(dt),
             mean=float(np.abs(mean - ref["mean"]).max() / np.abs(ref["mean"]).max()))
    hs = np.abs(ref["H"]).max(axis=1, keepdims=True)
    e["H"] = float((np.abs(H - ref["H"]) / np.where(hs > 0, hs, 1.0)).max())
    sd = np.sqrt(np.diag(ref["P"]))
    e["P"] = None if P is None else float((np.abs(P - ref["P"]) / np.outer(sd, sd)).max())
    e["whiten"] = float(np.abs(R @ ref["P"] @ R.T - np.eye(15)).max())
    e["R"] = float((np.abs(R - ref["R"]) / np.abs(ref["R"]).max(axis=1, keepdims=True)).max())
    return e
