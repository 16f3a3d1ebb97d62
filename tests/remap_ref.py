"""References of the COVARIANCE REMAPPING of a scan-matching Hessian (vf_degeneracy_remap_batch, k_remap_covariance), tests
only.  No GPU here.

The rule (include/vilfusion.h): Hs = (H + H^T) / 2, H' = D Hs D with D = diag(trans_thr^-1/2 x 3, rot_thr^-1/2 x 3),
H' = V diag(l') V^T, g_i = clamp(l'_i, floor, 1), Sigma = N + N^1/2 [sum_i (1 / g_i - 1) v_i v_i^T] N^1/2 with N = diag(nom6),
M = Sigma^-1 = N^-1/2 V diag(g) V^T N^-1/2, and eig = the eigenvalues of Hs, ascending.

  * `reference`: the rule in mpmath (mp.eigsy at 60 digits) -> Sigma_ref, M_ref, eig_ref as float64;
  * `evaluations`: three plain float64 evaluations -- numpy.linalg.eigh with both matrices in the additive form, the same in
    the product form, and a cyclic Jacobi written out in Python in the additive form;
  * `err`: entrywise, normalised by sqrt(ref_ii ref_jj); `eig_err`: normalised by max |eig_ref|;
  * the cases; S[case] = (S_cov, S_info, S_eig): the largest error over the evaluations, measured by
    tests/test_remap_ref_host.py, which asserts measured <= written <= 1.25 x measured;
  * the bar of the device: refine_ref.BAR_FACTOR x S + cov_ref.POSE_ROUNDING.  Nothing about it comes from a device result;
  * `mutations`: the rule wrong in one place, which the host test shows to land beyond 10 x the bar in at least one case each.

tests/test_remap_ref_host.py is what fixes the numbers; tests/test_gpu_remap.py holds the device to them."""
from __future__ import annotations

import functools

import mpmath as mp
import numpy as np

from tests import cov_ref as cr
from tests import refine_ref as rr
from vil_sensor_fusion_amd import synth
from vil_sensor_fusion_amd.degeneracy import ROT_DEGEN_THRESHOLD, TRANS_DEGEN_THRESHOLD, eigen_threshold

NOM6 = np.array([0.1, 0.1, 0.1, 0.2, 0.2, 0.2])
THR, FLOOR, SEED = 1e3, 1e-6, 5
TUNNEL = (0.4, 0.6, 1e-6)
SWAP = np.array([3, 4, 5, 0, 1, 2])             # [trans, rot] <-> [rot, trans]
BIG = [4e4, 5e4, 2.9e4, 4.4e4, 5.5e4]           # five eigenvalues well above the threshold


# ---------------------------------------------------------------- cases
def _q(rng, mix=1.0):
    return np.linalg.qr(rng.normal(size=(6, 6)) * mix + np.eye(6))[0]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (H (6, 6), trans_thr, rot_thr)}; nom6 = NOM6 and floor = FLOOR for all of them"""
    rng = np.random.default_rng(SEED)
    spec = lambda ev, q: (q * np.array(ev)) @ q.T
    qt = _q(rng)                                 # threshold+ and threshold- share their eigenvectors (continuity is tested on them)
    seq = synth.make_sequence(seed=42, n_kf=40, tunnel=TUNNEL)
    in_tunnel = np.nonzero(seq.tunnel[seq.loam_kf])[0]
    out = {
        "open": spec([3e4] + BIG, _q(rng)),
        "tunnel": spec([0.04] + BIG, _q(rng, 0.05)),
        "two equal": spec([5.0, 5.0] + BIG[1:], _q(rng)),
        "all equal": 10.0 * np.eye(6),
        "threshold+": spec([THR * (1 + 1e-9)] + BIG, qt),
        "threshold-": spec([THR * (1 - 1e-9)] + BIG, qt),
        "below floor": spec([1e-5, 0.0, -1e-3] + BIG[2:], _q(rng)),
        "graded": spec([1e-2, 1.0, 1e2, 1e4, 1e6, 1e8], _q(rng)),
        "diagonal": np.diag([0.04] + BIG),
    }
    out = {k: (0.5 * (h + h.T), THR, THR) for k, h in out.items()}
    out["split thresholds"] = (seq.loam_hessians[in_tunnel[0]], eigen_threshold(TRANS_DEGEN_THRESHOLD), eigen_threshold(ROT_DEGEN_THRESHOLD))
    return out


CASES = ("open", "tunnel", "two equal", "all equal", "threshold+", "threshold-", "below floor", "graded", "diagonal", "split thresholds")
DEWEIGHTED = {"open": 0, "tunnel": 1, "two equal": 2, "all equal": 6, "threshold+": 0, "threshold-": 1, "below floor": 3, "graded": 3,
              "diagonal": 1, "split thresholds": 1}
EXACTLY_NOMINAL = ("open", "threshold+")

# (S_cov, S_info, S_eig): the largest error over `evaluations`, as measured by tests/test_remap_ref_host.py (the value beside
# each entry), rounded up to two digits.  The test asserts measured <= written <= 1.25 x measured.
S = {
    "open":             (9.2e-16, 9.2e-16, 1.2e-15),   # measured 9.122e-16, 9.122e-16, 1.191e-15
    "tunnel":           (8.4e-13, 9.0e-14, 1.6e-15),   # measured 8.312e-13, 8.960e-14, 1.587e-15
    "two equal":        (1.9e-12, 3.4e-14, 5.3e-16),   # measured 1.848e-12, 3.307e-14, 5.292e-16
    "all equal":        (1.8e-16, 1.2e-15, 0.0),   # measured 1.776e-16, 1.110e-15, 0.000e+00
    "threshold+":       (1.2e-15, 1.2e-15, 9.3e-16),   # measured 1.131e-15, 1.131e-15, 9.260e-16
    "threshold-":       (3.5e-15, 3.6e-15, 1.2e-15),   # measured 3.469e-15, 3.553e-15, 1.191e-15
    "below floor":      (2.8e-15, 9.7e-15, 6.7e-16),   # measured 2.707e-15, 9.648e-15, 6.615e-16
    "graded":           (4.8e-07, 2.8e-11, 1.1e-15),   # measured 4.724e-07, 2.761e-11, 1.043e-15
    "diagonal":         (3.7e-16, 1.1e-12, 0.0),   # measured 3.638e-16, 1.000e-12, 0.000e+00
    "split thresholds": (4.7e-11, 1.7e-13, 8.9e-16),   # measured 4.661e-11, 1.604e-13, 8.820e-16
}


def bar(case):
    """(cov, info, eig)"""
    return tuple(rr.BAR_FACTOR * s + cr.POSE_ROUNDING for s in S[case])


# ---------------------------------------------------------------- the exact reference
def _d(trans_thr, rot_thr):
    return np.array([trans_thr] * 3 + [rot_thr] * 3) ** -0.5


def reference(H, nom6=NOM6, trans_thr=THR, rot_thr=THR, floor=FLOOR, dps=60):
    """(Sigma_ref, M_ref, eig_ref, deweighted) of the rule in mpmath at `dps` digits, rounded to float64 at the end"""
    with mp.workdps(dps):
        f = lambda x: mp.mpf(float(x))
        Hs = mp.matrix(6, 6)
        for i in range(6):
            for j in range(6):
                Hs[i, j] = (f(H[i, j]) + f(H[j, i])) / 2
        d = [1 / mp.sqrt(f(trans_thr))] * 3 + [1 / mp.sqrt(f(rot_thr))] * 3
        Hp = mp.matrix(6, 6)
        for i in range(6):
            for j in range(6):
                Hp[i, j] = Hs[i, j] * d[i] * d[j]
        E, Q = mp.eigsy(Hp)
        g = [min(max(E[k], f(floor)), mp.mpf(1)) for k in range(6)]
        s = [mp.sqrt(f(x)) for x in nom6]
        C, M = np.zeros((6, 6)), np.zeros((6, 6))
        for i in range(6):
            for j in range(6):
                C[i, j] = float((f(nom6[i]) if i == j else 0) + s[i] * s[j] * sum((1 / g[k] - 1) * Q[i, k] * Q[j, k] for k in range(6)))
                M[i, j] = float(sum(g[k] * Q[i, k] * Q[j, k] for k in range(6)) / (s[i] * s[j]))
        eig = np.sort([float(e) for e in mp.eigsy(Hs, eigvals_only=True)])
        return C, M, eig, int(sum(1 for k in range(6) if g[k] < 1))


# ---------------------------------------------------------------- float64 evaluations
def jacobi(A, sweeps=12):
    """(eigenvalues, V) of a symmetric matrix by cyclic two-sided Jacobi, every operation in float64"""
    A, n = np.array(A, dtype=np.float64), A.shape[0]
    V = np.eye(n)
    eps = np.finfo(np.float64).eps
    tiny = eps * eps * np.sum(A * A)
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if not apq * apq > eps * eps * max(abs(A[p, p] * A[q, q]), tiny):
                    continue
                rotated = True
                alpha = 0.5 * (A[q, q] - A[p, p])
                t = apq / np.copysign(abs(alpha) + np.hypot(alpha, apq), alpha)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                J = np.eye(n)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
        if not rotated:
            break
    return np.diag(A).copy(), V


def additive(lam, V, nom6, floor):
    """(Sigma, M) from the eigen-decomposition of H': both as corrections of the nominal"""
    g = np.clip(lam, floor, 1.0)
    s = np.sqrt(nom6)
    C = np.diag(nom6) + ((V * (1.0 / g - 1.0)) @ V.T) * np.outer(s, s)
    M = (np.eye(6) + (V * (g - 1.0)) @ V.T) / np.outer(s, s)
    return C, M


def product(lam, V, nom6, floor):
    g = np.clip(lam, floor, 1.0)
    s = np.sqrt(nom6)
    return ((V / g) @ V.T) * np.outer(s, s), ((V * g) @ V.T) / np.outer(s, s)


def evaluations(H, nom6=NOM6, trans_thr=THR, rot_thr=THR, floor=FLOOR):
    """{which: (Sigma, M, eig)}: three correct float64 evaluations of the rule"""
    Hs = 0.5 * (H + H.T)
    d = _d(trans_thr, rot_thr)
    Hp = Hs * np.outer(d, d)
    lam, V = np.linalg.eigh(Hp)
    lj, Vj = jacobi(Hp)
    return {"eigh, additive": (*additive(lam, V, nom6, floor), np.linalg.eigvalsh(Hs)),
            "eigh, product": (*product(lam, V, nom6, floor), np.sort(np.linalg.eigvals(Hs).real)),
            "jacobi, additive": (*additive(lj, Vj, nom6, floor), np.sort(jacobi(Hs)[0]))}


def err(A, R):
    d = np.sqrt(np.abs(np.diag(R)))
    return float(np.max(np.abs(A - R) / np.outer(d, d)))


def eig_err(e, ref):
    return float(np.max(np.abs(np.asarray(e) - ref)) / np.max(np.abs(ref)))


def info_of(sqrt_info21):
    """R^T R of the packed upper triangle"""
    R = np.zeros((6, 6))
    R[np.triu_indices(6)] = sqrt_info21
    return R.T @ R


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """what the tests of one case share: (Sigma_ref, M_ref, eig_ref, deweighted)"""
    H, tt, rt = cases()[name]
    return reference(H, NOM6, tt, rt, FLOOR)


def measure(name):
    """(S_cov, S_info, S_eig) measured, and the three evaluations' own errors"""
    H, tt, rt = cases()[name]
    C, M, E, _ = case_reference(name)
    errs = {k: (err(c, C), err(m, M), eig_err(e, E)) for k, (c, m, e) in evaluations(H, NOM6, tt, rt, FLOOR).items()}
    return tuple(max(v[i] for v in errs.values()) for i in range(3)), errs


# ---------------------------------------------------------------- mutations (the bar can fail)
def mutations(name):
    """{what: Sigma} of the rule wrong in one place (eigh, additive form)"""
    H, tt, rt = cases()[name]
    ev = lambda nom=NOM6, a=tt, b=rt, fl=FLOOR: evaluations(H, nom, a, b, fl)["eigh, additive"][0]
    lam, V = np.linalg.eigh(0.5 * (H + H.T) * np.outer(_d(tt, rt), _d(tt, rt)))
    g = np.clip(lam, FLOOR, 1.0)
    one_side = np.diag(NOM6) + ((V * (1.0 / g - 1.0)) @ V.T) * np.sqrt(NOM6)[None, :]
    return {"thresholds x 2": ev(a=2 * tt, b=2 * rt), "floor x 10": ev(fl=10 * FLOOR), "nom6 reversed": ev(nom=NOM6[::-1].copy()),
            "order swapped": ev()[np.ix_(SWAP, SWAP)], "N^1/2 on one side only": one_side}
