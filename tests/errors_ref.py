"""numpy reference of the per-window summaries and the batch health vf_engine_factor_errors leaves (include/vilfusion.h
vf_consistency, vf_batch_health), evaluated on the per-factor errors read back from the device.  Tests only."""
import math

import numpy as np

ROWS = (15, 6, 15, 27, 6, 6)
NONFINITE, FLAGGED, EMPTY = 1, 2, 4


def _klass(errs, idx, thr):
    """(count, sum, max, argmax, flagged, nonfinite) of one class: errs with -1 where there is no factor, idx their indices"""
    errs, idx = np.asarray(errs, dtype=np.float64), np.asarray(idx)
    there = ~(errs == -1.0)
    e, i = errs[there], idx[there]
    fin = np.isfinite(e)
    ef, jf = e[fin], i[fin]
    thr = float(thr) if thr is not None and math.isfinite(thr) and thr > 0 else math.inf
    if ef.size == 0:
        return int(e.size), 0.0, -1.0, -1, 0, int(e.size)
    m = float(ef.max())
    return int(e.size), float(math.fsum(ef)), m, int(jf[ef == m].min()), int(np.sum(2.0 * ef > thr)), int(e.size - ef.size)


def summary(imu, btw, k0, lo, hi, prior, marginal, far, far_linear, thresholds):
    """imu / btw: errors of keyframe slots k0 .. (any stretch that covers [lo, hi)); prior: (slot, error) or None; marginal: error
    or None; far / far_linear: the window's far arrays; thresholds: six or None"""
    t = [None] * 6 if thresholds is None else list(thresholds)
    slots = k0 + np.arange(len(imu))
    inside = (slots > lo) & (slots < hi)
    per = [_klass(np.asarray(imu)[inside], slots[inside], t[0]), _klass(np.asarray(btw)[inside], slots[inside], t[1]),
           _klass([prior[1]] if prior else [], [prior[0]] if prior else [], t[2]),
           _klass([marginal] if marginal is not None else [], [lo] if marginal is not None else [], t[3]),
           _klass(far, np.arange(len(far)), t[4]), _klass(far_linear, np.arange(len(far_linear)), t[5])]
    out = {name: [p[j] for p in per] for j, name in enumerate(("count", "sum", "max", "argmax", "flagged", "nonfinite"))}
    total = 0.0
    for s in out["sum"]:
        total += s                    # the six sums in class order, as the device adds them
    kf = max(hi - lo, 0)
    status = (NONFINITE if any(out["nonfinite"]) else 0) | (FLAGGED if any(out["flagged"]) else 0) | (EMPTY if hi <= lo else 0)
    out.update(total=total, keyframes=kf, rows=sum(r * c for r, c in zip(ROWS, out["count"])), unknowns=15 * kf, status=status)
    return out


def reduced_chi2(s):
    return 2.0 * s["total"] / float(max(s["rows"] - s["unknowns"], 1))


def health(summaries, costs, n_acc, n_fail):
    empty = [bool(s["status"] & EMPTY) for s in summaries]
    worst, value = -1, 0.0
    for w, s in enumerate(summaries):
        if not empty[w] and (worst < 0 or reduced_chi2(s) > value):
            worst, value = w, reduced_chi2(s)
    return dict(windows=len(summaries), empty=sum(empty), failed=sum(f > 0 for f in n_fail),
                nonfinite=sum((not math.isfinite(c)) or bool(s["status"] & NONFINITE) for c, s in zip(costs, summaries)),
                never_accepted=sum((not e) and a == 0 for e, a in zip(empty, n_acc)),
                flagged_windows=sum(bool(s["status"] & FLAGGED) for s in summaries), worst_window=worst, worst_reduced_chi2=value)
