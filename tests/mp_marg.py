"""Extended-precision reference of the fixed-lag marginalisation (k_marginalize / vfo_marginalize) and the componentwise
bound a float64 implementation of it has to stay within (tests only).

The operation.  The factors that touch the leaving keyframe m -- the IMU factor m -> m+1, the between factors m -> m+d
(d = 1, 2, 3; far factors that short are absorbed the same way), the anchor prior or the previous marginal prior -- form a
42 x 42 system A x = -b over [m: 15][m+1: 15][m+2 pose: 6][m+3 pose: 6]; the new marginal prior is the Schur complement of
m's 15 columns, S = A22 - A21 A11^-1 A12 (27 x 27, symmetrised), eta = b2 - A21 A11^-1 b1, over [m+1: 15][m+2 pose][m+3 pose].
A previous marginal prior (L, eta, xbar over [m: 15][m+1 pose][m+2 pose]) enters as A += L, b += L d + eta with d =
marg_delta (k2b_priors.inc): per keyframe j the Pose3 Logmap of xbar_j^-1 x_j, for j = 0 also v, ba, bg differences.

Inputs are float64 values taken exactly (a Case below); everything is evaluated with mpmath at mp_lie.DPS digits.

The bound (derived, never measured).  Beside the exact system the module carries F (42 x 43, last column = b): for every
entry the sum of |x_i| |x_j| over every product that forms it -- the quantity a floating-point sum's error is proportional
to, whatever its order.  Inputs that are themselves ROUNDED RESULTS of the code under test (the reference cannot take them
from the device exactly, or the code under test recomputes them) add their first-order uncertainty to F, in units of
u = 2^-53 so that the case's factor c multiplies them too:
  * marginal-prior gradient g = L d + eta: F_b += |L| |d| + |eta| (its formation) + |L| u_d.  d is computed by the code under
    test in float64: a quaternion product and a Log -- u_d = 4 |d|_inf of the pose's rotation part + 1 (one ulp of the O(1)
    quaternion components, absolute) on rotation components; u_d = 8 |t - tbar|_1 on translation components (R^T and
    J_l^-1 mix the three components of a difference that is itself exact to one rounding); u_d = |d| (one rounding of a
    difference) on v and the biases.
  * anchor prior rows taken from mp_lie.prior_factor because the device's have no reader (Case.prior with `rounded`): the
    pose rows are Log and J_r^-1 of the same quaternion product divided by sigma -- u_r = (8 |xi|_inf + 1) / sigma_i on the
    three rotation rows, 8 |xi|_inf / sigma_i on the translation rows (xi = the unwhitened 6-residual), u_J = 8 max|J sigma|
    / sigma_i on the structurally non-zero pose entries; the velocity / bias rows are (x - mean) / sigma and 1 / sigma: u_r =
    2 |r|, u_J = |J|.  A product J_ri J_rj then contributes u_J,ri |J_rj| + |J_ri| u_J,rj.
  * far factors absorbed like band factors, linearised by mp_lie.between_factor (Case.btw with `rounded`): the whitened rows
    are R (6 x 6 upper) times Log / LogmapDerivative blocks -- u = 16 max|block| per 6 x 6 block, (16 |r|_inf + |R|_max) for r.
Rows the code under test reads back exactly (Engine.read_imu_lin / read_between_lin, or the oracle's own linearisations on
the host) carry no uncertainty.

With the mpmath elimination of the 15 pivots, A11 = Lh D Lh^T continued over all 42 rows and the right-hand side (Lh: 42 x 15
unit lower trapezoid, U = D [Lh^T | y]: the pivot rows), W = A21 A11^-1 and z = A11^-1 b1:
    E = F + |Lh| |U|                                                          (42 x 43)
    B = E22 + |W| E12 + E21 |W|^T + |W| E11 |W|^T                             (27 x 27)
    B_eta = E2b + |W| E1b + E21 |z| + |W| E11 |z|                             (27)
the first-order componentwise bound of Gaussian elimination without pivoting (Higham, Accuracy and Stability, thm 9.3 / 10.3:
|dA| <= gamma |L| |U|), pushed through the Schur complement dS = dA22 - W dA12 - dA21 W^T + W dA11 W^T.
A computed entry passes when |got - ref| <= c 2^-53 B; where B == 0 (a structural zero) it must be exactly 0.
c (ops_bound) = the floating-point operations on the longest chain that can touch one entry: 15 IMU terms, 6 per between
factor present, 15 prior terms, 1 marginal-prior add, 3 per pivot (divide, multiply, subtract) x 15, 2 for the
symmetrisation -- rounded up to a power of two.  It is computed from the case, never fitted.

Gauge floor.  G (27 x 4): global translation (3 columns) and rotation about gravity, in the tangent frames of the three kept
keyframes, as the kernel's comment defines it; Q = its orthonormal basis (mpmath QR); M = Q^T S Q; lift = Q f(M) Q^T with
f(x) = max(floor_p - x, 0) through mp.eigsy; floor_p = gauge_floor n / 3.  The lift depends on span(G) only.  f is
Lipschitz-1 in the Frobenius norm, so an error dM of M moves the lift's 4 x 4 core by at most |dM|_F in every entry:
    dM  <= c u |Q|^T B |Q|  +  C_Q u |Q|^T |S| |Q|
    ext  = |Q| 1 1^T |Q|^T |dM|_F  +  C_Q u |Q| |f(M)| |Q|^T
C_Q = 512 >= 54 (two 27-term dot products per entry of M) + 216 (modified Gram-Schmidt of 4 columns of 27) + 240 (ten
Jacobi sweeps of six rotations).  The floored prior passes when |got - (S + lift)| <= c u B + ext."""
from __future__ import annotations

from dataclasses import dataclass, field

import mpmath as mp
import numpy as np

from tests import mp_lie as ml

U53 = mp.mpf(2) ** -53
C_Q = 512
IMU_COL = [c if c < 9 else c + 9 for c in range(15)] + [c + 9 if c < 9 else c + 15 for c in range(15)]   # 42-index (< 30) -> GTSAM column
OFF = {1: 15, 2: 30, 3: 36}                            # first 42-index of the pose of keyframe m + d
MAP27 = list(range(21)) + list(range(30, 36))          # index of the PREVIOUS marginal prior -> 42-index
KEEP = list(range(15, 42))


@dataclass
class Case:
    """inputs of one marginalisation, float64 taken exactly.
    imu = (r 15, J 15 x 30 in GTSAM column order); btw = [dict(d, r, Ja, Jb, rounded: bool, R: 6 x 6 or None)];
    prior = dict(r, J, sig, rounded) or None; marg = dict(L, eta, xbar 3 x 16) or None with `states` = the current states
    of m .. m+3 (4 x 16; needed for marg and the gauge floor)."""
    name: str
    imu: tuple
    btw: list = field(default_factory=list)
    prior: dict | None = None
    marg: dict | None = None
    states: np.ndarray | None = None
    n_kf: int = 4
    gravity: tuple = (0.0, 0.0, -9.81)


def ops_bound(case: Case) -> int:
    n = 15 + 6 * len(case.btw) + (15 if case.prior is not None else 0) + (1 if case.marg is not None else 0) + 3 * 15 + 2
    c = 1
    while c < n:
        c *= 2
    return c


# ---------------------------------------------------------------- row blocks: (42-columns, J, r, uJ, ur), mpf lists
def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return [[mp.mpf(float(v)) for v in row] for row in a]


def blocks_of(case: Case):
    out = []
    r, J = case.imu
    Jm = _mat(J)
    out.append(dict(kind="imu", cols=list(range(30)), J=[[row[IMU_COL[i]] for i in range(30)] for row in Jm], r=ml.vec(r), uJ=None, ur=None))
    for f in case.btw:
        ob = OFF[int(f["d"])]
        Ja, Jb = _mat(f["Ja"]), _mat(f["Jb"])
        Jrow = [Ja[i] + Jb[i] for i in range(6)]
        uJ = ur = None
        if f.get("rounded"):
            ma, mb = max(abs(v) for row in Ja for v in row), max(abs(v) for row in Jb for v in row)
            uJ = [[16 * ma] * 6 + [16 * mb] * 6 for _ in range(6)]
            rm = max(abs(mp.mpf(float(v))) for v in np.asarray(f["R"]).ravel())
            ur = [16 * max(abs(mp.mpf(float(v))) for v in f["r"]) + rm] * 6
        out.append(dict(kind="btw", cols=list(range(6)) + list(range(ob, ob + 6)), J=Jrow, r=ml.vec(f["r"]), uJ=uJ, ur=ur))
    if case.prior is not None:
        p = case.prior
        Jp, rp = _mat(p["J"]), ml.vec(p["r"])
        uJ = ur = None
        if p.get("rounded"):
            sig = ml.vec(p["sig"])
            xi = max(abs(rp[i] * sig[i]) for i in range(6))
            jm = max(abs(Jp[i][j] * sig[i]) for i in range(6) for j in range(6))
            uJ, ur = ml.zeros(15, 15), [mp.mpf(0)] * 15
            for i in range(6):
                ur[i] = (8 * xi + (1 if i < 3 else 0)) / sig[i]
                for j in range(3 if i < 3 else 6):
                    uJ[i][j] = 8 * jm / sig[i]
            for i in range(6, 15):
                ur[i] = 2 * abs(rp[i])
                uJ[i][i] = abs(Jp[i][i])
        out.append(dict(kind="prior", cols=list(range(15)), J=Jp, r=rp, uJ=uJ, ur=ur))
    return out


def marg_delta(marg, states):
    """(d 27, u_d 27) of k2b_priors.inc's marg_delta in mpmath; u_d in units of u (module docstring)"""
    d, ud = [mp.mpf(0)] * 27, [mp.mpf(0)] * 27
    for j in range(3):
        xb, x = ml.vec(marg["xbar"][j]), ml.vec(states[j])
        Rb = ml.quat_to_rot(xb[0:4])
        Rx = ml.quat_to_rot(x[0:4])
        dt = ml.vadd(x[4:7], xb[4:7], -1)
        w, u = ml.se3_log_Rt(ml.mm(ml.tr(Rb), Rx), ml.mv(ml.tr(Rb), dt))
        o = 0 if j == 0 else 15 + 6 * (j - 1)
        wm, t1 = max(abs(v) for v in w), mp.fsum(abs(v) for v in dt)
        for c in range(3):
            d[o + c], ud[o + c] = w[c], 4 * wm + 1
            d[o + 3 + c], ud[o + 3 + c] = u[c], 8 * t1
        if j == 0:
            for c in range(9):
                d[6 + c] = x[7 + c] - xb[7 + c]
                ud[6 + c] = abs(d[6 + c])
    return d, ud


def form(case: Case):
    """(A 42 x 42, b 42, F 42 x 43) in mpmath"""
    A, b, F = ml.zeros(42, 42), [mp.mpf(0)] * 42, ml.zeros(42, 43)
    for blk in blocks_of(case):
        cols, J, r, uJ, ur = blk["cols"], blk["J"], blk["r"], blk["uJ"], blk["ur"]
        nr = len(J)
        for a, ia in enumerate(cols):
            ca = [J[k][a] for k in range(nr)]
            if not any(ca) and uJ is None:
                continue
            ua = [uJ[k][a] for k in range(nr)] if uJ is not None else None
            for c, ic in enumerate(cols):
                cc = [J[k][c] for k in range(nr)]
                A[ia][ic] += mp.fsum(x * y for x, y in zip(ca, cc))
                F[ia][ic] += mp.fsum(abs(x * y) for x, y in zip(ca, cc))
                if ua is not None:
                    F[ia][ic] += mp.fsum(ua[k] * abs(cc[k]) + abs(ca[k]) * uJ[k][c] for k in range(nr))
            b[ia] += mp.fsum(x * y for x, y in zip(ca, r))
            F[ia][42] += mp.fsum(abs(x * y) for x, y in zip(ca, r))
            if ua is not None:
                F[ia][42] += mp.fsum(ua[k] * abs(r[k]) + abs(ca[k]) * ur[k] for k in range(nr))
    if case.marg is not None:
        L, eta = _mat(case.marg["L"]), ml.vec(case.marg["eta"])
        d, ud = marg_delta(case.marg, case.states)
        for i in range(27):
            for j in range(27):
                A[MAP27[i]][MAP27[j]] += L[i][j]
                F[MAP27[i]][MAP27[j]] += abs(L[i][j])
            b[MAP27[i]] += mp.fsum(L[i][j] * d[j] for j in range(27)) + eta[i]
            F[MAP27[i]][42] += mp.fsum(abs(L[i][j]) * (abs(d[j]) + ud[j]) for j in range(27)) + abs(eta[i])
    return A, b, F


def eliminate(A, b, F):
    """Schur complement of the 15 leading columns and its bound: dict(S 27 x 27, eta 27, B 27 x 27, Beta 27), mpf lists"""
    n = 42
    T = [list(A[i]) + [b[i]] for i in range(n)]           # working copy, augmented
    Lh = ml.zeros(n, 15)
    Up = ml.zeros(15, 43)
    for c in range(15):
        piv = T[c][c]
        if not piv > 0:
            raise ArithmeticError(f"pivot {c} of the reference is not positive")
        Up[c] = [T[c][j] if j >= c else mp.mpf(0) for j in range(43)]
        for i in range(c, n):
            Lh[i][c] = T[i][c] / piv
        for i in range(c + 1, n):
            l = Lh[i][c]
            if l == 0:
                continue
            for j in range(c + 1, 43):
                T[i][j] -= l * T[c][j]
    S = [[(T[15 + i][15 + j] + T[15 + j][15 + i]) / 2 for j in range(27)] for i in range(27)]
    eta = [T[15 + i][42] for i in range(27)]
    E = [[F[i][j] + mp.fsum(abs(Lh[i][c] * Up[c][j]) for c in range(15)) for j in range(43)] for i in range(n)]
    A11 = mp.matrix([[A[i][j] for j in range(15)] for i in range(15)])
    rhs = mp.matrix([[A[i][15 + j] for j in range(27)] + [b[i]] for i in range(15)])
    X = mp.inverse(A11) * rhs                             # 15 x 28: [W^T | z]
    Wa = [[abs(X[k, i]) for k in range(15)] for i in range(28)]        # |W| rows 0..26, |z| row 27
    E11 = [[E[i][j] for j in range(15)] for i in range(15)]
    WE11 = [[mp.fsum(Wa[i][k] * E11[k][l] for k in range(15)) for l in range(15)] for i in range(27)]
    B = ml.zeros(27, 27)
    Beta = [mp.mpf(0)] * 27
    for i in range(27):
        for j in range(28):
            col = 15 + j if j < 27 else 42
            v = E[15 + i][col] + mp.fsum(Wa[i][k] * E[k][col] for k in range(15))
            v += mp.fsum((E[15 + i][k] + WE11[i][k]) * Wa[j][k] for k in range(15))
            if j < 27:
                B[i][j] = v
            else:
                Beta[i] = v
    B = [[max(B[i][j], B[j][i]) for j in range(27)] for i in range(27)]
    return dict(S=S, eta=eta, B=B, Beta=Beta)


def reference(case: Case):
    out = eliminate(*form(case))
    out["c"] = ops_bound(case)
    return out


# ---------------------------------------------------------------- gauge floor
def gauge_basis(states3, gravity):
    """Q 27 x 4 (mpf lists): orthonormal basis of the span of G, built from the kept keyframes' states (m+1, m+2, m+3)"""
    g = ml.vec(gravity)
    gn = mp.sqrt(ml.dot(g, g))
    ez = [-v / gn for v in g] if gn > 0 else [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    G = ml.zeros(27, 4)
    x0 = ml.vec(states3[0])
    for j in range(3):
        x = ml.vec(states3[j])
        o = 0 if j == 0 else 15 + 6 * (j - 1)
        R = ml.quat_to_rot(x[0:4])
        lever = ml.cross(ez, ml.vadd(x[4:7], x0[4:7], -1))
        for c in range(3):
            for a in range(3):
                G[o + 3 + c][a] = R[a][c]
            G[o + c][3] = mp.fsum(R[a][c] * ez[a] for a in range(3))
            G[o + 3 + c][3] = mp.fsum(R[a][c] * lever[a] for a in range(3))
        if j == 0:
            ev = ml.cross(ez, x[7:10])
            for c in range(3):
                G[6 + c][3] = ev[c]
    Q, _ = mp.qr(mp.matrix(G), mode="skinny")
    return [[Q[i, a] for a in range(4)] for i in range(27)]


def floor_lift(ref, Q, floor_p):
    """(lift 27 x 27, ext 27 x 27, eigenvalues of M, |dM|_F): the gauge floor's lift of ref['S'] and the extra admissible
    error.  Where every eigenvalue exceeds floor_p by more than |dM|_F no admissible M reaches the floor: the lift is zero
    for the code under test as well, and ext is None (the plain bound holds)."""
    S, B, c = ref["S"], ref["B"], ref["c"]
    Qa = [[abs(v) for v in row] for row in Q]
    M = ml.mm(ml.tr(Q), ml.mm(S, Q))
    M = [[(M[a][b] + M[b][a]) / 2 for b in range(4)] for a in range(4)]
    ev, V = mp.eigsy(mp.matrix(M))
    fl = mp.mpf(floor_p)
    fv = [max(fl - ev[e], mp.mpf(0)) for e in range(4)]
    fM = [[mp.fsum(V[a, e] * fv[e] * V[b, e] for e in range(4)) for b in range(4)] for a in range(4)]
    lift = ml.mm(Q, ml.mm(fM, ml.tr(Q)))
    Sa = [[abs(v) for v in row] for row in S]
    dM = ml.add(ml.scal(c * U53, ml.mm(ml.tr(Qa), ml.mm(B, Qa))), ml.scal(C_Q * U53, ml.mm(ml.tr(Qa), ml.mm(Sa, Qa))))
    dMF = mp.sqrt(mp.fsum(v * v for row in dM for v in row))
    rs = [mp.fsum(row) for row in Qa]
    fMa = [[abs(v) for v in row] for row in fM]
    core = ml.mm(Qa, ml.mm(fMa, ml.tr(Qa)))
    ext = [[rs[i] * rs[j] * dMF + C_Q * U53 * core[i][j] for j in range(27)] for i in range(27)]
    evs = [ev[e] for e in range(4)]
    if min(evs) - dMF > fl:
        return None, None, evs, dMF
    return lift, ext, evs, dMF


def floor_properties(got_L, ref, Q, ext, floor_p, rng):
    """what the floored prior L (float64) must satisfy beside L = S + lift: returns (eigenvalues of Q^T L Q, the admissible
    shortfall below floor_p -- the admissible error of L carried into the 4 x 4, Frobenius --, worst |L v - S v| / bound over
    four random v orthogonal to Q: the lift acts on span(Q) only)"""
    Qa = [[abs(v) for v in row] for row in Q]
    L = _mat(got_L)
    tol = [[ref["c"] * U53 * ref["B"][i][j] + ext[i][j] for j in range(27)] for i in range(27)]
    M = ml.mm(ml.tr(Q), ml.mm(L, Q))
    ev = mp.eigsy(mp.matrix([[(M[a][b] + M[b][a]) / 2 for b in range(4)] for a in range(4)]), eigvals_only=True)
    dM = ml.mm(ml.tr(Qa), ml.mm(tol, Qa))
    slack = mp.sqrt(mp.fsum(v * v for row in dM for v in row))
    worst = mp.mpf(0)
    for _ in range(4):
        v = ml.vec(rng.normal(size=27))
        for a in range(4):
            qa = [Q[i][a] for i in range(27)]
            v = ml.vadd(v, qa, -ml.dot(v, qa))
        Lv, Sv = ml.mv(L, v), ml.mv(ref["S"], v)
        bound = ml.mv(tol, [abs(x) for x in v])
        worst = max(worst, max(abs(Lv[i] - Sv[i]) / bound[i] for i in range(27)))
    return [ev[e] for e in range(4)], slack, float(worst)


# ---------------------------------------------------------------- comparison
def worst_ratio(got, ref, bound, c, ext=None):
    """max over entries of |got - ref| / (c u bound + ext) -- inf where the bound is 0 and the entry is not exactly 0;
    got: float64 array, ref / bound: mpf lists of the same shape (1-D or 2-D).  Also returns the entry."""
    got = np.asarray(got, dtype=np.float64)
    worst, where = mp.mpf(0), None
    for idx in np.ndindex(got.shape):
        r, bd = ref, bound
        for k in idx:
            r, bd = r[k], bd[k]
        tol = c * U53 * bd
        if ext is not None:
            e = ext
            for k in idx:
                e = e[k]
            tol += e
        err = abs(mp.mpf(float(got[idx])) - r)
        if tol == 0:
            ratio = mp.mpf(0) if (err == 0 and float(got[idx]) == 0.0) else mp.inf
        else:
            ratio = err / tol
        if ratio > worst:
            worst, where = ratio, idx
    return float(worst), where


def check(case_name, got_L, got_eta, ref, what="", lift=None, ext=None):
    """prints the worst |err| / (c 2^-53 B) of L and eta (the headroom) and returns them; the caller asserts <= 1"""
    S = ref["S"] if lift is None else ml.add(ref["S"], lift)
    rl, wl = worst_ratio(got_L, S, ref["B"], ref["c"], ext)
    re_, we = worst_ratio(got_eta, ref["eta"], ref["Beta"], ref["c"])
    print(f"{what}{case_name}: c = {ref['c']}, worst |err| / (c 2^-53 B): L {rl:.3e} at {wl}, eta {re_:.3e} at {we}")
    return rl, re_
