"""References of the LOOP-CLOSURE GATE (vf_engine_gate_closures, kernels/kclosure.inc), tests only.  No GPU here.

For a window [lo, hi) and a candidate BetweenFactor<Pose3> between two of its keyframes a < b:

    Sigma_J  = [[Sigma_aa^pp, Sigma_ab^pp], [Sigma_ba^pp, Sigma_bb^pp]]      pose dofs 0..5 of the keyframes' 15, of
               Sigma = (J^T J + L)^-1 at lambda = 0 of everything the window holds (tests/cov_ref.py)
    r, Ja, Jb  the whitened between factor at (x_a, x_b); xi its unwhitened residual [rot, trans]
    S        = I + [Ja Jb] Sigma_J [Ja Jb]^T, symmetrised
    nis      = r^T S^-1 r,   nis_measurement = r^T r

This module builds on tests/cov_ref.py (cases, exact_cov, evaluations, err's normalisation) and tests/gate_ref.py (measurement,
the mpmath arithmetic, the float64 Cholesky) and adds

  * `candidates`: the fixed candidate list of every case of cov_ref.CASES, at most four on a window;
  * `joint`, `err_joint`: Sigma_J of a dense Sigma, and max |Sigma_J - ref| / sqrt(ref_ii ref_jj) over its 144 entries;
  * `nis_mp`: extended precision (mpmath at mp_lie's 50 digits) from a float64 Sigma_J taken as exact input;
  * `nis_f64`: the same statement in numpy on the CPU oracle;
  * S_JOINT, the floor of Sigma_J: the largest err_joint over cov_ref.evaluations and the case's candidates; the device's bar is
    refine_ref.BAR_FACTOR x S_JOINT.  NIS_FLOOR: the worst relative error of nis_f64 fed the reference Sigma_J; the device's nis
    bar is 16 x that.  Nothing about a bar comes from a device result;
  * `mutations`: Sigma_J (or nis) wrong in one way, which tests/test_closure_ref_host.py shows to land beyond 10 x the bar, or
    records as blind.

tests/test_closure_ref_host.py is what fixes the numbers; tests/test_gpu_closure_gate.py holds the device to them."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import cov_ref as cr
from tests import direct_ref as dr
from tests import gate_ref, mp_lie
from tests import refine_ref as rr

KINDS = ("consistent", "gross")
COV36 = gate_ref.cov36()
FAR_PAIR = dr.FAR17[0]                     # F17, G17: the candidate on a live far factor's own pair of keyframes
POSE12 = lambda a, b: [15 * a + d for d in range(6)] + [15 * b + d for d in range(6)]      # noqa: E731


def candidates(case):
    """[(a, b)] in absolute keyframe numbers: (lo, hi-1), (lo, lo+1), (hi-2, hi-1), from six keyframes on (lo+1, hi-2) -- the cap of
    four -- without repeats; L1: the degenerate (lo, lo) alone; F17 and G17: FAR_PAIR in place of the fourth (the cap holds)"""
    lo, hi = case.lo, case.hi
    if case.n == 1:
        return [(lo, lo)]
    out = [(lo, hi - 1), (lo, lo + 1), (hi - 2, hi - 1)]
    if case.n >= 6:
        out.append(FAR_PAIR if case.far is not None else (lo + 1, hi - 2))
    seen = []
    for c in out:
        if c not in seen:
            seen.append(c)
    return seen


def testable(case):
    return [(a, b) for a, b in candidates(case) if a < b]


def joint(Sigma, a, b):
    """Sigma_J (12, 12) of window-local keyframes a, b of a dense Sigma"""
    ix = POSE12(a, b)
    return Sigma[np.ix_(ix, ix)]


def err_joint(J, Jref):
    d = np.sqrt(np.diag(Jref))
    return float(np.max(np.abs(J - Jref) / np.outer(d, d)))


def record(oracle, case, a, b, kind):
    return gate_ref.measurement(oracle, case.states[a], case.states[b], COV36, kind)


def mp_factor(rec28, x_a, x_b):
    """the part of nis_mp that does not depend on Sigma_J: (r 6 x 1, [Ja Jb] 6 x 12 as mpmath matrices, xi (6,) float64)"""
    rw, Ja, Jb = mp_lie.between_factor(rec28, x_a, x_b)
    xi = mp_lie.between_factor(rec28, x_a, x_b, whiten=False)[0]
    return gate_ref._mpm(rw.reshape(6, 1)), gate_ref._mpm(np.hstack([Ja, Jb])), xi


def nis_mp(rec28, x_a, x_b, SJ, factor=None):
    """dict nis, nis_measurement (float64, rounded once), xi (6,): mpmath from the float64 Sigma_J taken as exact input"""
    rw, J, xi = mp_factor(rec28, x_a, x_b) if factor is None else factor
    S = mp.eye(6) + J * gate_ref._mpm(SJ) * J.T
    S = (S + S.T) / 2
    y = mp.lu_solve(S, rw)
    return dict(nis=float((rw.T * y)[0, 0]), nis_measurement=float((rw.T * rw)[0, 0]), xi=xi)


def nis_f64(oracle, rec28, x_a, x_b, SJ, swap=False):
    """the same in float64 numpy on the CPU oracle (swap: Ja and Jb exchanged, a mutation)"""
    r, Ja, Jb = oracle.between_factor(rec28, x_a, x_b)
    J = np.hstack([Jb, Ja] if swap else [Ja, Jb])
    S = np.eye(6) + J @ SJ @ J.T
    S = 0.5 * (S + S.T)
    return dict(nis=gate_ref._chol_solve_quadratic(S, r), nis_measurement=float(r @ r), xi=oracle.between_factor(rec28, x_a, x_b, whiten=False)[0])


# S_JOINT: the largest err_joint over cov_ref.evaluations and the case's candidates, as measured by tests/test_closure_ref_host.py
# (the value beside each entry), rounded up to two digits.  The test asserts measured <= written <= 1.25 x measured.
S_JOINT = {
    "L1":   None,      # the degenerate (lo, lo) alone: nothing can be tested
    "L2":   5.0e-15,   # measured 4.963e-15
    "L3":   7.7e-15,   # measured 7.649e-15
    "L4":   2.1e-14,   # measured 2.022e-14
    "L5":   1.1e-13,   # measured 1.080e-13
    "L7":   2.7e-13,   # measured 2.693e-13
    "L8":   1.2e-12,   # measured 1.181e-12
    "L9":   7.7e-13,   # measured 7.606e-13
    "L15":  1.9e-11,   # measured 1.891e-11
    "L16":  2.6e-11,   # measured 2.570e-11
    "L17":  5.5e-11,   # measured 5.485e-11
    "L24":  2.1e-10,   # measured 2.022e-10
    "L25":  7.0e-10,   # measured 6.971e-10
    "L26":  7.8e-10,   # measured 7.728e-10
    "L33":  2.0e-09,   # measured 1.923e-09
    "L34":  2.2e-09,   # measured 2.133e-09
    "L35":  4.7e-09,   # measured 4.659e-09
    "P3":   2.3e-11,   # measured 2.288e-11
    "P13":  5.1e-09,   # measured 5.087e-09
    "M12":  2.1e-11,   # measured 2.003e-11
    "F17":  5.5e-11,   # measured 5.468e-11
    "G17":  2.6e-11,   # measured 2.542e-11
}
# NIS_FLOOR: the worst relative error of nis_f64 fed the reference Sigma_J against nis_mp, over every case, candidate and kind, as
# measured by tests/test_closure_ref_host.py (measured <= written <= 1.25 x measured)
NIS_FLOOR = 4.6e-13      # measured 4.515e-13 (P3, (3, 19), consistent)
NIS_BAR = 16.0 * NIS_FLOOR
# xi: 7e-15 per component, absolute (the float64 restatement stays within 1.8e-15 of mpmath on every case).  nis_measurement = |R xi|^2,
# R the record's square-root information: an xi within XI_BAR moves it by at most 2 |r| |R|_2 sqrt(6) XI_BAR to first order, and its
# own six products and sums add 16 eps relative -- `measurement_bar`.  (A relative bar of 7e-15 would ask more of |r|^2 than float64
# gives: the consistent measurements lie 0.3 sigma from the prediction, where xi is a small difference of poses.)
XI_BAR = 7e-15
EPS = np.finfo(np.float64).eps


def measurement_bar(rec28, nis_measurement):
    R = np.zeros((6, 6))
    R[np.triu_indices(6)] = np.asarray(rec28)[7:28]
    return 2.0 * np.sqrt(nis_measurement) * np.linalg.norm(R, 2) * np.sqrt(6.0) * XI_BAR + 16.0 * EPS * nis_measurement


# mutations that do NOT land beyond 10 x the bar: {(case, mutation, (a, b)): multiple of the bar}, measured by
# tests/test_closure_ref_host.py (measured <= written <= 1.25 x measured)
BLIND = {
}


def bar(name):
    return rr.BAR_FACTOR * S_JOINT[name]


def reference(oracle, f, nis=True, floors=True):
    """f: cov_ref.reference of a case.  {(a, b): dict(SJ reference Sigma_J, recs {kind: record}, factor {kind: mp_factor}; with
    floors: errs {evaluation: err_joint}; with nis: mp {kind: nis_mp fed SJ}, f64 {kind: nis_f64 fed SJ})}, and with floors the
    case's S_JOINT measured (else None).  The GPU tests need neither the floors nor the CPU's own nis"""
    case = f["case"]
    ev = cr.evaluations(oracle, case, f["rows"]) if floors else {}
    out = {}
    for a, b in testable(case):
        SJ = joint(f["Sref"], a - case.lo, b - case.lo)
        recs = {k: record(oracle, case, a, b, k) for k in KINDS}
        xa, xb = case.states[a], case.states[b]
        c = dict(SJ=SJ, errs={k: err_joint(joint(x, a - case.lo, b - case.lo), SJ) for k, x in ev.items()}, recs=recs,
                 factor={k: mp_factor(r, xa, xb) for k, r in recs.items()})
        if nis:
            c["mp"] = {k: nis_mp(r, xa, xb, SJ, c["factor"][k]) for k, r in recs.items()}
            c["f64"] = {k: nis_f64(oracle, r, xa, xb, SJ) for k, r in recs.items()}
        out[(a, b)] = c
    s = max((max(c["errs"].values()) for c in out.values()), default=None) if floors else None
    return out, s


def mutations(oracle, f, cref):
    """[(name, (a, b), multiple of the Sigma_J bar or of the nis bar)] of one case"""
    case, name = f["case"], f["case"].name
    rw = f["rows"]
    out = []
    band = cr.band_inverse(oracle, dr.normal_from_rows(rw)[0]) if case.far is not None else None
    nomp = None
    if case.marg is not None:
        nomp = cr.dense_inverse(rr.band_dense(dr.normal_from_rows(rr.Rows(rw.J, rw.r, np.zeros_like(rw.L), rw.g_mp, rw.blocks))[0]))
    for (a, b), c in cref.items():
        SJ, la, lb = c["SJ"], a - case.lo, b - case.lo
        T = SJ.copy()
        T[:6, 6:], T[6:, :6] = SJ[:6, 6:].T, SJ[6:, :6].T
        out.append(("Sigma_ab transposed", (a, b), err_joint(T, SJ) / bar(name)))
        Z = SJ.copy()
        Z[:6, 6:] = Z[6:, :6] = 0.0
        out.append(("Sigma_ab zeroed", (a, b), err_joint(Z, SJ) / bar(name)))
        if band is not None:
            out.append(("the downdate left out", (a, b), err_joint(joint(band, la, lb), SJ) / bar(name)))
        if nomp is not None:
            m = err_joint(joint(nomp, la, lb), SJ) / bar(name) if np.all(np.isfinite(nomp)) else np.inf
            out.append(("the marginal prior left out", (a, b), m))
        for k in KINDS:
            sw = nis_f64(oracle, c["recs"][k], case.states[a], case.states[b], SJ, swap=True)["nis"]
            out.append((f"Ja and Jb swapped, {k}", (a, b), abs(sw - c["mp"][k]["nis"]) / c["mp"][k]["nis"] / NIS_BAR))
    return out
