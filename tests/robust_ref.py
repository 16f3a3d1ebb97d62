"""References of the robust losses on between factors (include/vilfusion.h "Robust loss on band between factors"; the device code
is vil_sensor_fusion_amd/csrc/vf_robust.hpp and robustify_between of csrc/kernels/k12_linearize.inc).  Tests only.

  1. the scalar functions alpha(s) = sqrt(2 rho) / s and gamma(s) = alpha' / s at 100 digits, FROM THE DEFINITION of rho (no
     closed form of alpha or gamma is typed in here), and three float64 evaluations of each in algebraically different forms;
  2. the square-root form of a factor, r^ = alpha r and J^ = (alpha I + gamma r r^T) J, at 100 digits from given doubles, three
     float64 evaluations of it, and the entry-wise normalised error;
  3. the cases the GPU tests run (tests/test_gpu_robust.py) and the host test holds to their conditions
     (tests/test_robust_ref_host.py);
  4. dense host optimisers of the robust cost: IRLS in GTSAM's form (sqrt(w) r, sqrt(w) J) and Gauss-Newton on the square-root
     form.

Bars are 16 S, S the largest error three correct float64 evaluations have against the extended-precision value."""
from __future__ import annotations

import functools
import math

import mpmath as mp
import numpy as np

NONE, HUBER, CAUCHY, GM = 0, 1, 2, 3
LOSSES = (HUBER, CAUCHY, GM)
NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", GM: "geman_mcclure"}
DPS = 100
EPS = 2.0 ** -52


# ---------------------------------------------------------------- 1. scalars
def mp_rho(loss, k, s):
    k, s = mp.mpf(k), mp.mpf(s)
    if loss == NONE or (loss == HUBER and s <= k):
        return s * s / 2
    if loss == HUBER:
        return k * (s - k / 2)
    if loss == CAUCHY:
        return k * k / 2 * mp.log(1 + s * s / (k * k))
    return k * k * s * s / (2 * (k * k + s * s))


def mp_drho(loss, k, s):
    """rho'(s)"""
    k, s = mp.mpf(k), mp.mpf(s)
    if loss == NONE or (loss == HUBER and s <= k):
        return s
    if loss == HUBER:
        return k
    if loss == CAUCHY:
        return s * k * k / (k * k + s * s)
    return s * k ** 4 / (k * k + s * s) ** 2


def mp_alpha_gamma(loss, k, s):
    """(alpha, gamma) from rho and rho' alone: alpha = sqrt(2 rho) / s, alpha' = rho' / (s sqrt(2 rho)) - sqrt(2 rho) / s^2.  The two
    terms of alpha' cancel to u = s^2 / k^2 of their size: 100 digits keep 64 at u = 1e-18."""
    with mp.workdps(DPS):
        k, s = mp.mpf(k), mp.mpf(s)
        q = mp.sqrt(2 * mp_rho(loss, k, s))
        return q / s, (mp_drho(loss, k, s) / (s * q) - q / (s * s)) / s


def _cauchy_g_taylor(u):            # -1/2 + 2 u / 3 - 3 u^2 / 4 + ..., u < 0.03
    t = 0.0
    for n in range(15, -1, -1):
        t = t * u + (-1.0) ** (n + 1) * (n + 1.0) / (n + 2.0)
    return t


def _cauchy_g_w(u):                 # log1p(u) - u / (1 + u) = -log(1 - w) - w = sum_{n >= 2} w^n / n, w = u / (1 + u) <= 1 / 2: all positive
    w = u / (1.0 + u)
    t = 0.0
    for n in range(70, 1, -1):
        t = t * w + 1.0 / n
    return -(t * w * w) / (u * u)


_GL_X, _GL_W = np.polynomial.legendre.leggauss(48)


def _cauchy_g_quad(u):              # g(u) = -int_0^1 x / (1 + u x)^2 dx (log1p(u) - u / (1 + u) = int_0^u v / (1 + v)^2 dv, v = u x)
    x = 0.5 * (_GL_X + 1.0)
    return -0.5 * float(np.sum(_GL_W * x / (1.0 + u * x) ** 2))


def _cauchy_g_atanh(u):             # the device's form, restated
    z = u / (2.0 + u)
    t = 0.0
    for n in range(17, -1, -1):
        t = t * z * z + 1.0 / (2 * n + 3)
    return -0.5 * (1.0 - z) ** 2 * (1.0 / (1.0 + z) + z * t)


def forms(loss):
    """three float64 evaluations (s, k) -> (alpha, gamma), algebraically different; Huber: s > k"""
    if loss == HUBER:
        def a(s, k):
            q = math.sqrt(k * (2.0 * s - k))
            return q / s, -k * (s - k) / (s ** 3 * q)

        def b(s, k):
            t = k / s
            q = math.sqrt(t * (2.0 - t))
            return q, -t * ((s - k) / s) / (s * s * q)

        def c(s, k):
            return math.sqrt(2.0 * k * (s - 0.5 * k)) / s, -(s - k) / (s * s * s * math.sqrt(2.0 * s / k - 1.0))
        return a, b, c
    if loss == CAUCHY:
        def a(s, k):
            u = (s / k) ** 2
            al = math.sqrt(math.log1p(u) / u)
            g = _cauchy_g_atanh(u) if u <= 1.0 else (u / (1.0 + u) - math.log1p(u)) / (u * u)
            return al, g / (al * k * k)

        def b(s, k):
            u = (s / k) ** 2
            al = math.sqrt(math.log1p(u)) / (s / k)
            g = _cauchy_g_taylor(u) if u < 0.03 else (_cauchy_g_w(u) if u <= 1.0 else (u / (1.0 + u) - math.log1p(u)) / (u * u))
            return al, g / (k * k) / al

        def c(s, k):
            u = (s / k) ** 2
            al = math.sqrt(2.0 * math.atanh(u / (2.0 + u)) / u) if u <= 1.0 else math.sqrt(k * k * math.log1p(u)) / s      # (atanh near 1 is ill-conditioned)
            g = _cauchy_g_quad(u) if u <= 1.0 else (1.0 / (1.0 + u) - math.log1p(u) / u) / u
            return al, g / al / (k * k)
        return a, b, c

    def a(s, k):
        u = (s / k) ** 2
        return 1.0 / math.sqrt(1.0 + u), -1.0 / ((1.0 + u) ** 1.5 * k * k)

    def b(s, k):
        h = math.hypot(k, s)
        return k / h, -k / h ** 3

    def c(s, k):
        al = math.sqrt(1.0 / (1.0 + (s / k) ** 2))
        return al, -al ** 3 / (k * k)
    return a, b, c


GRID_K = (1.345, 0.01, 37.0)


def scalar_grid(loss):
    """(s, k): u = s^2 / k^2 from 1e-18 to 1e12 in quarter decades for three k, s = k and s = k (1 +- 2^-52); Huber keeps s > k"""
    pts = []
    for k in GRID_K:
        for i in range(0, 121):
            pts.append((k * math.sqrt(10.0 ** (-18.0 + 0.25 * i)), k))
        pts += [(k, k), (k * (1.0 + EPS), k), (k * (1.0 - EPS / 2), k), (k * (1.0 + 2.0 ** -30), k)]
    return [(s, k) for s, k in pts if loss != HUBER or s > k]


def rel(got, want):
    with mp.workdps(DPS):
        return float(abs((mp.mpf(got) - want) / want)) if want != 0 else (0.0 if got == 0 else math.inf)


@functools.lru_cache(maxsize=None)
def scalar_reference(loss):
    return [mp_alpha_gamma(loss, k, s) for s, k in scalar_grid(loss)]


@functools.lru_cache(maxsize=None)
def scalar_S():
    """largest relative error of the three float64 forms of alpha and gamma over the grids of the three losses"""
    worst = 0.0
    for loss in LOSSES:
        for (s, k), (al, ga) in zip(scalar_grid(loss), scalar_reference(loss)):
            for f in forms(loss):
                a, g = f(s, k)
                worst = max(worst, rel(a, al), rel(g, ga))
    return worst


def split(x):
    """an mpf as two doubles (hi, lo), 106 bits"""
    with mp.workdps(DPS):
        hi = float(x)
        return hi, float(x - mp.mpf(hi))


# ---------------------------------------------------------------- 2. the square-root form of a factor
def mp_hat(r, J, loss, k):
    """(r^ (6,), J^ (6, c), alpha, gamma) as mp values from the doubles r (6,), J (6, c); a slot without a loss and a Huber inlier:
    the factor itself, alpha = 1, gamma = 0"""
    with mp.workdps(DPS):
        rm = [mp.mpf(float(x)) for x in r]
        Jm = [[mp.mpf(float(x)) for x in row] for row in np.asarray(J)]
        s = mp.sqrt(sum(x * x for x in rm))
        if loss == NONE or (loss == HUBER and s <= mp.mpf(k)):
            return rm, Jm, mp.mpf(1), mp.mpf(0)
        if s == 0:
            return rm, Jm, mp.mpf(1), mp.mpf(0)          # r = 0: r^ = 0 and J^ = J whatever gamma is
        al, ga = mp_alpha_gamma(loss, k, s)
        cols = len(Jm[0])
        dots = [sum(rm[l] * Jm[l][j] for l in range(6)) for j in range(cols)]
        return [al * x for x in rm], [[al * Jm[i][j] + ga * rm[i] * dots[j] for j in range(cols)] for i in range(6)], al, ga


def hat_forms(r, J, loss, k):
    """three float64 evaluations of (r^, J^); the norm is sqrt(r . r) in float64 in each"""
    r, J = np.asarray(r, dtype=np.float64), np.asarray(J, dtype=np.float64)
    s = math.sqrt(float(r @ r))
    if loss == NONE or (loss == HUBER and s <= k) or s == 0.0:
        return [(r.copy(), J.copy())] * 3
    fa, fb, fc = forms(loss)
    out = []
    a, g = fa(s, k)
    out.append((a * r, a * J + g * np.outer(r, r @ J)))
    a, g = fb(s, k)
    out.append((a * r, (a * np.eye(6) + g * np.outer(r, r)) @ J))
    a, g = fc(s, k)
    out.append((a * r, a * (J + np.outer(r * (g / a), r @ J))))
    return out


def hat_error(got_r, got_J, r, J, loss, k, want=None):
    """largest entry-wise error of (got_r, got_J) against mp_hat(r, J), every entry normalised by the size of what it is made of:
    |alpha| |r_i| for r^, |alpha| |J_ij| + |gamma| |r_i| sum_l |r_l J_lj| for J^ (an entry made of nothing must be exact)"""
    with mp.workdps(DPS):
        rh, Jh, al, ga = want if want is not None else mp_hat(r, J, loss, k)
        worst = 0.0
        for i in range(6):
            n = abs(al) * abs(mp.mpf(float(r[i])))
            d = abs(mp.mpf(float(got_r[i])) - rh[i])
            worst = max(worst, float(d / n) if n != 0 else (0.0 if d == 0 else math.inf))
            for j in range(len(Jh[0])):
                n = abs(al) * abs(mp.mpf(float(J[i][j]))) + abs(ga) * abs(mp.mpf(float(r[i]))) * sum(abs(mp.mpf(float(r[l])) * mp.mpf(float(J[l][j]))) for l in range(6))
                d = abs(mp.mpf(float(got_J[i][j])) - Jh[i][j])
                e = float(d / n) if n != 0 else (0.0 if d == 0 else math.inf)
                worst = max(worst, e if math.isfinite(e) or not math.isnan(float(got_J[i][j])) else math.inf)
        return worst


def near_threshold(loss, ratio):
    """a Huber factor whose norm is within rounding distance of k: gamma is proportional to s - k, which the float64 norm leaves with
    few correct bits -- the float64 evaluations differ there by orders of magnitude more than anywhere else, and so may the device.
    (Where J_ij is a structural zero -- the isotropic records' rotation rows against translation columns -- J^_ij is the gamma term
    alone, and so is its normaliser: the error of s - k shows there undiluted by the alpha term.)"""
    return loss == HUBER and ratio is not None and abs(ratio - 1.0) < 1e-3


def near_threshold_cap(ratio):
    """what such a factor's own S may be at most: the float64 norm (six multiply-adds and a square root) is within 4 eps of s, so
    s - k, and gamma with it, within 4 eps s / |s - k| = 4 eps / |1 - k / s|; twice that.  An own S beyond it is no rounding."""
    return 8.0 * EPS / abs(1.0 - 1.0 / ratio)


def hat_S(r, J, loss, k):
    """largest normalised error of the three float64 evaluations for these doubles"""
    want = mp_hat(r, J, loss, k)
    return max(hat_error(rh, Jh, r, J, loss, k, want) for rh, Jh in hat_forms(r, J, loss, k))


def weight_condition(loss, k, s):
    """|d ln w / d ln e| of the weight w = rho'/s as a function of the error e = rho(s): how much robust.weight_from_error amplifies
    a relative error of e.  Huber: w = k / s, s = e / k + k / 2.  Cauchy: w = exp(-2 e / k^2).  Geman-McClure: w = (1 - 2 e / k^2)^2,
    which saturates: the error of a far outlier no longer says how far out it is."""
    if loss == NONE or (loss == HUBER and s <= k) or s == 0.0:
        return 0.0
    if loss == HUBER:
        return (k * (s - 0.5 * k)) / (k * s)
    u = (s / k) ** 2
    if loss == CAUCHY:
        return math.log1p(u)
    return 2.0 * u


def gtsam_form(r, J, loss, k):
    """GTSAM's reweighted factor (sqrt(w) r, sqrt(w) J), float64"""
    from vil_sensor_fusion_amd import robust
    w = math.sqrt(robust.weight(loss, k, math.sqrt(float(np.dot(r, r)))))
    return w * np.asarray(r), w * np.asarray(J)


# ---------------------------------------------------------------- 3. cases
B, CAPACITY, SLOT0 = 3, 128, 59          # three windows; the keyframes start at slot 59 so that the range crosses the AoSoA tile boundary at 64
LIN_N, OPT_N = 10, 8
LIN_SEEDS, OPT_SEEDS = (11, 12, 13), (21, 22, 23)
# what the factors of a linearisation window are given, in the order of their end keyframes: (loss, s / k); s / k = None: r = 0 exactly
LIN_PLAN = (
    [(HUBER, 0.5), (CAUCHY, 50.0), (NONE, 1.0), (GM, 1.0), (HUBER, 50.0), (CAUCHY, 0.5), (GM, 1e6), (HUBER, 1.0 - 2.0 ** -30), (NONE, 1.0), (CAUCHY, 1.0)],
    [(GM, 0.5), (HUBER, 1e6), (CAUCHY, 1.0), (NONE, 1.0), (GM, 50.0), (HUBER, 0.5), (CAUCHY, 1e6), (GM, 1.0), (HUBER, 50.0), (NONE, 1.0)],
    [(CAUCHY, None), (HUBER, None), (GM, None), (NONE, 1.0), (HUBER, 1.0 + 2.0 ** -30), (CAUCHY, 50.0), (GM, 1e6), (HUBER, 3.0), (CAUCHY, 0.5), (GM, 50.0)],
)
OUTLIER = {HUBER: (6.0, 1.345), CAUCHY: (6.0, 2.3849), GM: (6.0, 2.0)}     # optimum cases: metres the outlier increment is off by, and k
OPT_TRIALS = 60


def _problem(oracle, seed, n, perturb):
    from tests import helpers
    from vil_sensor_fusion_amd import synth
    seq = synth.make_sequence(seed=seed, n_kf=n)
    return helpers.build_problem(oracle, seq, perturb=perturb)


@functools.lru_cache(maxsize=None)
def _lin_cases_cached():
    from oracle import oracle
    oracle.build()
    out = []
    for w in range(B):
        prob = _problem(oracle, LIN_SEEDS[w], LIN_N, 0.02)
        states = prob["states"].copy()
        plan, loss, k = LIN_PLAN[w], [], []
        for f, (a, b, rec) in enumerate(zip(prob["btw_a"], prob["btw_b"], prob["btw"])):
            ls, ratio = plan[f % len(plan)]
            if ratio is None:
                # r = 0 exactly: both poses and the measurement are exact binary numbers with identity rotations.  (The keyframes'
                # other factors then have residuals of any size: this case reads linearisations, it solves nothing.)
                for kf in (a, b):
                    states[kf, :7] = [1.0, 0.0, 0.0, 0.0, 1.0 + 0.5 * kf, 2.0 + 0.25 * kf, 3.0]
                prob["btw"][f, :7] = [1.0, 0.0, 0.0, 0.0, 0.5 * (b - a), 0.25 * (b - a), 0.0]
                loss.append(ls)
                k.append(1.5)
                continue
            loss.append(ls)
            k.append(ratio)              # (turned into k = s / ratio below, once every state is final)
        for f, (a, b, rec) in enumerate(zip(prob["btw_a"], prob["btw_b"], prob["btw"])):
            if plan[f % len(plan)][1] is not None:
                r, _, _ = oracle.between_factor(rec, states[a], states[b])
                k[f] = float(np.linalg.norm(r)) / k[f] if loss[f] != NONE else 0.0
        out.append(dict(prob=prob, states=states, loss=np.array(loss, dtype=np.int32), k=np.array(k),
                        ratio=[plan[f % len(plan)][1] for f in range(len(loss))]))
    return out


def lin_cases():
    """per window: prob, states (LIN_N, 16), and loss / k per between factor (in the order of prob["btw_b"])"""
    return _lin_cases_cached()


@functools.lru_cache(maxsize=None)
def _opt_cases_cached(loss):
    from oracle import oracle
    oracle.build()
    out = []
    for w in range(B):
        clean = _problem(oracle, OPT_SEEDS[w], OPT_N, 0.01)
        prob = dict(clean, btw=clean["btw"].copy())
        m = prob["btw_a"].size
        bad = (2 + w) % m
        off, k = OUTLIER[loss]
        prob["btw"][bad, 4:7] += np.array([off, -0.5 * off, 0.25 * off])
        ls = np.zeros(m, dtype=np.int32)
        ks = np.zeros(m)
        for f in range(m):                      # the outlier and every other factor carry the loss, the rest are Gaussian
            if f == bad or f % 2 == w % 2:
                ls[f], ks[f] = loss, k
        start = prob["states"].copy()
        if loss != HUBER:                       # the non-convex losses start at the Gaussian optimum of the clean data
            start = optimise(oracle, clean, clean["states"], np.zeros(m, dtype=np.int32), np.zeros(m), form="irls")[0]
        out.append(dict(prob=prob, clean=clean, start=start, loss=ls, k=ks, bad=bad))
    return out


def opt_cases(loss):
    return _opt_cases_cached(loss)


# ---------------------------------------------------------------- 4. host optimisers
def _rows(oracle, prob, states):
    from tests import refine_ref as rr
    return rr.rows(oracle, rr.Case("robust", prob, np.asarray(states), 0, prob["n"], 0))


def _btw_blocks(prob, rw):
    """[(factor index, first row)] of the between factors in the order of prob["btw_b"]"""
    blocks = [blk for blk in rw.blocks if blk[0] == "btw"]
    assert len(blocks) == prob["btw_a"].size
    return [(f, blk[3]) for f, blk in enumerate(blocks)]


def robust_rows(oracle, prob, states, loss, k, form):
    """(J, r) of the whole window with every robust between factor in GTSAM's form ("irls") or the square-root form ("sqrt")"""
    from vil_sensor_fusion_amd import robust
    rw = _rows(oracle, prob, states)
    J, r = rw.J.copy(), rw.r.copy()
    for f, row0 in _btw_blocks(prob, rw):
        if loss[f] == NONE:
            continue
        sl = slice(row0, row0 + 6)
        rb, Jb = r[sl].copy(), J[sl].copy()
        s = math.sqrt(float(rb @ rb))
        if (loss[f] == HUBER and s <= k[f]) or s == 0.0:
            continue
        if form == "irls":
            w = math.sqrt(robust.weight(int(loss[f]), k[f], s))
            r[sl], J[sl] = w * rb, w * Jb
        else:
            a, g = forms(int(loss[f]))[0](s, k[f])
            r[sl], J[sl] = a * rb, a * Jb + g * np.outer(rb, rb @ Jb)
    return J, r


def addends(oracle, prob, states, loss, k):
    """the cost's addends at `states`: 0.5 r_i^2 of every whitened row, a robust factor's rows as r^ = alpha r (their sum is rho(s))"""
    _, r = robust_rows(oracle, prob, states, loss, k, "sqrt")
    return 0.5 * r * r


def cost(oracle, prob, states, loss, k):
    return math.fsum(addends(oracle, prob, states, loss, k))


def optimise(oracle, prob, start, loss, k, form="irls", steps=200, tol=1e-13):
    """Levenberg-Marquardt on the dense rows (QR least squares, damping only when a step raises the cost) until the increment is below
    `tol` in every component; returns (states, cost, steps taken)"""
    states = np.asarray(start, dtype=np.float64).copy()
    n = prob["n"]
    c = cost(oracle, prob, states, loss, k)
    lam, small = 0.0, 0
    for it in range(steps):
        J, r = robust_rows(oracle, prob, states, loss, k, form)
        A = J if lam == 0.0 else np.vstack([J, math.sqrt(lam) * np.eye(J.shape[1])])
        b = -r if lam == 0.0 else np.concatenate([-r, np.zeros(J.shape[1])])
        d = np.linalg.lstsq(A, b, rcond=None)[0].reshape(n, 15)
        trial = np.array([oracle.retract(states[i], d[i]) for i in range(n)])
        ct = cost(oracle, prob, trial, loss, k)
        size = float(np.max(np.abs(d)))
        if ct <= c or size < tol:
            states, c = trial, min(c, ct)
            lam = lam / 10.0 if lam > 1e-12 else 0.0
            small = small + 1 if size < tol else 0
            if small >= 2:
                return states, c, it + 1
        else:
            lam = 1e-6 if lam == 0.0 else lam * 10.0
    raise AssertionError("the host optimiser did not converge")


@functools.lru_cache(maxsize=None)
def optima(loss, w):
    """the optimum of optimum case (loss, w) three ways -- IRLS, Gauss-Newton on the square-root form, IRLS from a perturbed start --
    the Gaussian optimum of the same data, and S = the largest distance between the positions of the three"""
    from oracle import oracle
    oracle.build()
    c = opt_cases(loss)[w]
    a = optimise(oracle, c["prob"], c["start"], c["loss"], c["k"], "irls")[0]
    b = optimise(oracle, c["prob"], c["start"], c["loss"], c["k"], "sqrt")[0]
    rng = np.random.default_rng(100 + w)
    moved = np.array([oracle.retract(s, rng.normal(size=15) * 1e-4) for s in a])
    d = optimise(oracle, c["prob"], moved, c["loss"], c["k"], "irls")[0]
    m = c["loss"].size
    gauss = optimise(oracle, c["prob"], c["start"], np.zeros(m, dtype=np.int32), np.zeros(m), "irls")[0]
    S = max(float(np.max(np.linalg.norm(x[:, 4:7] - y[:, 4:7], axis=1))) for x, y in ((a, b), (a, d), (b, d)))
    return dict(irls=a, sqrt=b, moved=d, gauss=gauss, S=S)


def position_error(x, y):
    return float(np.max(np.linalg.norm(np.asarray(x)[:, 4:7] - np.asarray(y)[:, 4:7], axis=1)))
