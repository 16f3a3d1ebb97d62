"""High-precision reference of the SO(3) / SE(3) / NavState math the kernels and the CPU oracle evaluate (tests only).

Everything is evaluated with mpmath at DPS significant digits from the float64 inputs exactly as the code under test receives
them: a coefficient takes the double x = theta^2 (theta = sqrt(x) in mpmath), a rotation takes the double quaternion or the
double rotation vector.  Nothing is re-derived from a nominal angle, so a one-ulp change of an input that the code under
test sees is seen here too.  Closed forms are evaluated at DPS + GUARD digits, which absorbs their cancellation at small
angles (the tiniest nonzero angle the tests use is 1e-12 rad: dE's closed form then loses 48 digits).

Definitions (DESIGN.md "Conventions"; GTSAM's Rot3 / Pose3 / NavState):
  Exp(w) = I + A W + B W^2, J_r(w) = I - B W + C W^2, J_r^{-1}(w) = I + W/2 + E W^2, J_l(w) = I + B W + C W^2
  A = sin/th, B = (1-cos)/th^2, C = (th-sin)/th^3, dB = B'(th)/th, dC = C'(th)/th,
  E = 1/th^2 - cot(th/2)/(2 th), dE = E'(th)/th
  Pose3 retract = full Expmap: (R Exp(w), t + R J_l(w) v); Logmap: (Log R, J_l(w)^{-1} t), tangent order [omega, v]
  Pose3 LogmapDerivative: Log(T Exp(d)) = Log(T) + J d + O(d^2), here by central differences in mpmath
  NavState retract (R Exp(dth), t + R dp, v + R dv), localCoordinates (Log(R^T R'), R^T (t' - t), R^T (v' - v))
  factor Jacobians by central differences over oracle.retract's chart (Pose3 Expmap, vector add for v and bias)."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 50
GUARD = 60
mp.mp.dps = DPS
H_FD = mp.mpf("1e-20")   # central-difference step: truncation ~H^2, rounding ~10^-DPS / H; both far below float64


def _m(a):
    return a if isinstance(a, mp.mpf) else mp.mpf(float(a))


def vec(a):
    return [_m(v) for v in np.asarray(a, dtype=np.float64).ravel()]


def to_np(a):
    """nested lists of mpf -> float64 array (round to nearest)"""
    if isinstance(a, (list, tuple)):
        return np.array([to_np(v) for v in a], dtype=np.float64)
    return float(a)


# ---------------------------------------------------------------- small dense algebra on lists
def zeros(n, m):
    return [[mp.mpf(0)] * m for _ in range(n)]


def eye(n):
    Z = zeros(n, n)
    for i in range(n):
        Z[i][i] = mp.mpf(1)
    return Z


def mm(A, B):
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def mv(A, v):
    return [mp.fsum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def tr(A):
    return [list(r) for r in zip(*A)]


def add(A, B, s=1):
    return [[a + s * b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def scal(s, A):
    return [[s * a for a in r] for r in A]


def vadd(a, b, s=1):
    return [x + s * y for x, y in zip(a, b)]


def dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def hat(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


# ---------------------------------------------------------------- coefficients of x = theta^2 (x: the double the code sees)
def coefs(x):
    """dict A, B, C, dB, dC, E, dE at the double x"""
    x = _m(x)
    if x == 0:
        return dict(A=mp.mpf(1), B=mp.mpf(1) / 2, C=mp.mpf(1) / 6, dB=-mp.mpf(1) / 12, dC=-mp.mpf(1) / 60,
                    E=mp.mpf(1) / 12, dE=mp.mpf(1) / 360)
    with mp.workdps(DPS + GUARD):
        th = mp.sqrt(x)
        s, c = mp.sin(th), mp.cos(th)
        A = s / th
        B = (1 - c) / x
        C = (th - s) / (x * th)
        dB = (A - 2 * B) / x
        dC = (B - 3 * C) / x
        h = th / 2
        E = 1 / x - mp.cot(h) / (2 * th)
        # E'(th) = -2/th^3 + cot(h)/(2 th^2) + 1/(4 th sin^2 h)
        dE = -2 / (x * x) + mp.cot(h) / (2 * x * th) + 1 / (4 * x * mp.sin(h) ** 2)
        out = dict(A=A, B=B, C=C, dB=dB, dC=dC, E=E, dE=dE)
    return {k: +v for k, v in out.items()}


# ---------------------------------------------------------------- SO(3)
def so3_exp_w(w):
    """w: list of mpf"""
    x = dot(w, w)
    with mp.workdps(DPS + GUARD):
        if x == 0:
            A, B = mp.mpf(1), mp.mpf(1) / 2
        else:
            th = mp.sqrt(x)
            A, B = mp.sin(th) / th, (1 - mp.cos(th)) / x
    W = hat(w)
    return add(add(eye(3), scal(A, W)), scal(B, mm(W, W)))


def quat_w(w):
    """Exp as a unit quaternion (cos(th/2), sin(th/2) w/th)"""
    x = dot(w, w)
    with mp.workdps(DPS + GUARD):
        if x == 0:
            return [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]
        th = mp.sqrt(x)
        k = mp.sin(th / 2) / th
        return [+mp.cos(th / 2), +(k * w[0]), +(k * w[1]), +(k * w[2])]


def quat_to_rot(q):
    """rotation of a not necessarily unit quaternion (w, x, y, z): that of q/|q| (as vfo_quat_to_rot / qrot)"""
    w, x, y, z = q
    s = 2 / (w * w + x * x + y * y + z * z)
    return [[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
            [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
            [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]]


def rot_to_quat(R):
    """Shepperd's method (well conditioned at every angle), w >= 0"""
    t = R[0][0] + R[1][1] + R[2][2]
    d = [t, R[0][0], R[1][1], R[2][2]]
    i = max(range(4), key=lambda k: d[k])
    if i == 0:
        s = 2 * mp.sqrt(1 + t)
        q = [s / 4, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s]
    elif i == 1:
        s = 2 * mp.sqrt(1 + R[0][0] - R[1][1] - R[2][2])
        q = [(R[2][1] - R[1][2]) / s, s / 4, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s]
    elif i == 2:
        s = 2 * mp.sqrt(1 + R[1][1] - R[0][0] - R[2][2])
        q = [(R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, s / 4, (R[1][2] + R[2][1]) / s]
    else:
        s = 2 * mp.sqrt(1 + R[2][2] - R[0][0] - R[1][1])
        q = [(R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, s / 4]
    n = mp.sqrt(dot(q, q))
    sg = -1 if q[0] < 0 else 1
    return [sg * v / n for v in q]


def quat_log(q):
    """Log of the rotation of q/|q|, angle in [0, pi]"""
    if q[0] < 0:
        q = [-v for v in q]
    n = mp.sqrt(q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
    if n == 0:
        return [mp.mpf(0)] * 3
    f = 2 * mp.atan2(n, q[0]) / n
    return [f * q[1], f * q[2], f * q[3]]


def so3_log_R(R):
    return quat_log(rot_to_quat(R))


def so3_jr_w(w):
    k = _coefs_mp(w)
    W = hat(w)
    return add(add(eye(3), scal(-k["B"], W)), scal(k["C"], mm(W, W)))


def _coefs_mp(w):
    """coefficients at the exact |w|^2 of an mpf vector (for maps whose input is the vector, not x)"""
    x = dot(w, w)
    if x == 0:
        return coefs(0.0)
    with mp.workdps(DPS + GUARD):
        th = mp.sqrt(x)
        s, c = mp.sin(th), mp.cos(th)
        A, B, C = s / th, (1 - c) / x, (th - s) / (x * th)
        h = th / 2
        E = 1 / x - mp.cot(h) / (2 * th)
        dB, dC = (A - 2 * B) / x, (B - 3 * C) / x
    return dict(A=+A, B=+B, C=+C, E=+E, dB=+dB, dC=+dC)


def so3_jr_inv_w(w):
    k = _coefs_mp(w)
    W = hat(w)
    return add(add(eye(3), scal(mp.mpf(1) / 2, W)), scal(k["E"], mm(W, W)))


def so3_jl_w(w):
    k = _coefs_mp(w)
    W = hat(w)
    return add(add(eye(3), scal(k["B"], W)), scal(k["C"], mm(W, W)))


def so3_jr_apply_dtheta_w(th, c):
    """d/dtheta [J_r(theta) c] for fixed c, by central differences"""
    D = zeros(3, 3)
    for j in range(3):
        e = [mp.mpf(0)] * 3
        e[j] = H_FD
        p = mv(so3_jr_w(vadd(th, e)), c)
        m = mv(so3_jr_w(vadd(th, e, -1)), c)
        for i in range(3):
            D[i][j] = (p[i] - m[i]) / (2 * H_FD)
    return D


# ---------------------------------------------------------------- SE(3)
def se3_exp_w(w, v):
    return so3_exp_w(w), mv(so3_jl_w(w), v)


def se3_log_Rt(R, t):
    w = so3_log_R(R)
    return w, se3_u(w, t)


def se3_u(w, t):
    """J_l(w)^{-1} t = (I - W/2 + E W^2) t"""
    k = _coefs_mp(w)
    W = hat(w)
    Vi = add(add(eye(3), scal(-mp.mpf(1) / 2, W)), scal(k["E"], mm(W, W)))
    return mv(Vi, t)


def se3_log_q(q, t):
    """Logmap of (rotation of the quaternion q, translation t)"""
    w = quat_log(q)
    return w, se3_u(w, t)


def se3_jr_inv_xi(w, u):
    """Pose3::LogmapDerivative at xi = [w, u]: Log(Exp(xi) Exp(d)) by central differences in d"""
    R, t = se3_exp_w(w, u)
    J = zeros(6, 6)
    for j in range(6):
        cols = []
        for s in (1, -1):
            d = [mp.mpf(0)] * 6
            d[j] = s * H_FD
            dR, dt = se3_exp_w(d[:3], d[3:])
            w2, u2 = se3_log_Rt(mm(R, dR), vadd(t, mv(R, dt)))
            cols.append(w2 + u2)
        for i in range(6):
            J[i][j] = (cols[0][i] - cols[1][i]) / (2 * H_FD)
    return J


# ---------------------------------------------------------------- states (16 doubles: q, t, v, bias acc, bias gyro)
class State:
    def __init__(self, R, t, v, b):
        self.R, self.t, self.v, self.b = R, t, v, b

    @staticmethod
    def of(x16):
        x = vec(x16)
        return State(quat_to_rot(x[0:4]), x[4:7], x[7:10], x[10:16])

    def to_np(self):
        return np.concatenate([to_np(rot_to_quat(self.R)), to_np(self.t), to_np(self.v), to_np(self.b)])


def retract_s(s: State, d):
    """oracle.retract's chart: Pose3 Expmap on d[0:6], add on v (d[6:9]) and bias (d[9:15]); d: mpf list"""
    dR, dt = se3_exp_w(d[0:3], d[3:6])
    return State(mm(s.R, dR), vadd(s.t, mv(s.R, dt)), vadd(s.v, d[6:9]), vadd(s.b, d[9:15]))


def retract(x16, d15):
    """mp result of oracle.retract(x, d) for double inputs, as a State"""
    return retract_s(State.of(x16), vec(d15))


def upper(Rp, n):
    R = zeros(n, n)
    o = 0
    for r in range(n):
        for c in range(r, n):
            R[r][c] = Rp[o]
            o += 1
    return R


def _fd(fun, states, cols):
    """central-difference Jacobian of fun(*states) (a list of mpf) over retract_s of the (state index, tangent slice) cols"""
    r0 = fun(*states)
    J = zeros(len(r0), sum(sl.stop - sl.start for _, sl in cols))
    c = 0
    for which, sl in cols:
        for k in range(sl.start, sl.stop):
            out = []
            for sg in (1, -1):
                d = [mp.mpf(0)] * 15
                d[k] = sg * H_FD
                st = list(states)
                st[which] = retract_s(states[which], d)
                out.append(fun(*st))
            for i in range(len(r0)):
                J[i][c] = (out[0][i] - out[1][i]) / (2 * H_FD)
            c += 1
    return r0, J


# ---------------------------------------------------------------- factors
def between_residual(rec, sa: State, sb: State, whiten=True):
    Rm = quat_to_rot(vec(rec[0:4]))
    tm = vec(rec[4:7])
    Rh = mm(tr(sa.R), sb.R)
    th = mv(tr(sa.R), vadd(sb.t, sa.t, -1))
    Re = mm(tr(Rm), Rh)
    te = mv(tr(Rm), vadd(th, tm, -1))
    w, u = se3_log_Rt(Re, te)
    r = w + u
    return mv(upper(vec(rec[7:28]), 6), r) if whiten else r


def between_factor(rec, xa, xb, whiten=True):
    """(r 6, Ja 6x6, Jb 6x6) as float64 arrays, Jacobians by central differences"""
    sa, sb = State.of(xa), State.of(xb)
    f = lambda a, b: between_residual(rec, a, b, whiten)
    r, J = _fd(f, [sa, sb], [(0, slice(0, 6)), (1, slice(0, 6))])
    J = to_np(J)
    return to_np(r), J[:, :6], J[:, 6:]


def prior_residual(rec, s: State):
    Rp = quat_to_rot(vec(rec[0:4]))
    te = mv(tr(Rp), vadd(s.t, vec(rec[4:7]), -1))
    w, u = se3_log_Rt(mm(tr(Rp), s.R), te)
    mean = vec(rec[0:16])
    sig = vec(rec[16:31])
    rest = vadd(s.v, mean[7:10], -1) + vadd(s.b, mean[10:16], -1)
    return [v / sg for v, sg in zip(w + u + rest, sig)]


def prior_factor(rec, x):
    r, J = _fd(lambda s: prior_residual(rec, s), [State.of(x)], [(0, slice(0, 15))])
    return to_np(r), to_np(J)


def _pim_predict(rec, g, si: State, bias):
    """PreintegrationBase::predict: bias-corrected delta, NavState::correctPIM (no Coriolis), NavState::retract"""
    r = vec(rec)
    dt, d, bhat, H = r[0], r[1:10], r[10:16], [r[16 + 6 * i:22 + 6 * i] for i in range(9)]
    inc = vadd(bias, bhat, -1)
    bc = vadd(d, mv(H, inc))
    RiT = tr(si.R)
    rv, rg = mv(RiT, si.v), mv(RiT, g)
    dt22 = dt * dt / 2
    xi = bc[0:3] + [bc[3 + i] + dt * rv[i] + dt22 * rg[i] for i in range(3)] + [bc[6 + i] + dt * rg[i] for i in range(3)]
    R = mm(si.R, so3_exp_w(xi[0:3]))
    return State(R, vadd(si.t, mv(si.R, xi[3:6])), vadd(si.v, mv(si.R, xi[6:9])), list(si.b))


def predict(rec, gravity, x16):
    """vfo_predict / k_predict: pose and velocity of the prediction, bias copied; float64 state (q with w >= 0)"""
    si = State.of(x16)
    return _pim_predict(rec, vec(gravity), si, si.b).to_np()


def imu_residual(rec, g, si: State, sj: State, whiten=True):
    pj = _pim_predict(rec, g, si, si.b)
    RjT = tr(sj.R)
    e = so3_log_R(mm(RjT, pj.R)) + mv(RjT, vadd(pj.t, sj.t, -1)) + mv(RjT, vadd(pj.v, sj.v, -1))
    ru = e + vadd(si.b, sj.b, -1)
    return mv(upper(vec(rec[70:190]), 15), ru) if whiten else ru


def imu_factor(rec, gravity, xi, xj, whiten=True):
    """(r 15, J 15x30); J's columns as vfo_imu_factor: [pose_i, vel_i, pose_j, vel_j, bias_i, bias_j]"""
    g = vec(gravity)
    f = lambda a, b: imu_residual(rec, g, a, b, whiten)
    cols = [(0, slice(0, 6)), (0, slice(6, 9)), (1, slice(0, 6)), (1, slice(6, 9)), (0, slice(9, 15)), (1, slice(9, 15))]
    r, J = _fd(f, [State.of(xi), State.of(xj)], cols)
    return to_np(r), to_np(J)


def imu_residual_only(rec, gravity, xi, xj, whiten=True):
    return to_np(imu_residual(rec, vec(gravity), State.of(xi), State.of(xj), whiten))


def preintegrate_mean(steps, bhat):
    """TangentPreintegration::update's mean over steps (dt, acc xyz, gyro xyz): returns (dt, [theta, p, v]) as float64"""
    T, d = preintegrate_mean_mp(steps, vec(bhat))
    return float(T), to_np(d)


def preintegrate_mean_mp(steps, b):
    """preintegrate_mean for a bias estimate b given as 6 mpf (so that it can be perturbed): (dt, [theta, p, v]) in mpf"""
    th, p, v = [mp.mpf(0)] * 3, [mp.mpf(0)] * 3, [mp.mpf(0)] * 3
    T = mp.mpf(0)
    for st in np.asarray(steps, dtype=np.float64):
        dt = _m(st[0])
        acc = vadd(vec(st[1:4]), b[0:3], -1)
        om = vadd(vec(st[4:7]), b[3:6], -1)
        wt = mv(so3_jr_inv_w(th), om)
        an = mv(so3_exp_w(th), acc)
        dt22 = dt * dt / 2
        p = [p[i] + v[i] * dt + an[i] * dt22 for i in range(3)]
        v = [v[i] + an[i] * dt for i in range(3)]
        th = [th[i] + wt[i] * dt for i in range(3)]
        T += dt
    return T, th + p + v


# ---------------------------------------------------------------- edge inputs shared by the host and the device tests
# rotation angles around every switch of vf_math.hpp / vf_oracle.c: 0, the qlog switch (|vec q| < 1e-7, theta ~ 2e-7), the
# qexp switch (x < 1e-4, theta = 0.01), the series switch of A..dE (x < 0.25, theta = 0.5), and the approach to pi where
# 1 + cos(theta) cancels.  Exactly pi is left out of residuals: the sign of the axis there is a free choice.
EDGE_ANGLES = [0.0, 1e-12, 1e-8, 1.9e-7, 2.1e-7, 0.00999, 0.01001, 0.1, 0.4999999, 0.5000001, 0.51, 1.3, 2.0, 2.9,
               np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-8]
# accumulated tangent angles of a preintegration (K0's theta is not wrapped): past pi, towards 2 pi
ABOVE_PI = [3.5, 5.0, 6.0]


def axis(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def band(angle):
    """name of the switch region an angle falls in (for the per-band error tables)"""
    if angle < 2e-7:
        return "qlog series (<2e-7)"
    if angle < 0.01:
        return "qexp series (<0.01)"
    if angle < 0.5:
        return "Horner (<0.5)"
    if angle < 3.0:
        return "closed form (0.5..3)"
    if angle < np.pi:
        return "near pi"
    return "above pi"


def coef_sensitivity(x):
    """|theta d/dtheta| of every coefficient at the double x (by central differences in mpmath): how far one relative
    rounding of theta = sqrt(x), or of the argument of a sin / cos, moves the coefficient in units of eps"""
    x = _m(x)
    if x == 0:
        return {k: mp.mpf(0) for k in coefs(0.0)}
    d = mp.mpf("1e-15")
    with mp.workdps(DPS + GUARD):
        p = coefs(x * (1 + d) ** 2)
        m = coefs(x * (1 - d) ** 2)
    return {k: abs(p[k] - m[k]) / (2 * d) for k in p}
