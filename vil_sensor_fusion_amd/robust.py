"""Robust losses on between factors (include/vilfusion.h "Robust loss on band between factors"): names and ids, and the scalar
functions of a loss as host arithmetic on numbers the device has computed -- what a caller needs to read a factor's
down-weighting off Engine.read_factor_errors / GraphManager.factor_errors.  Conventions of GTSAM's mEstimator classes: s is the
norm of the whitened residual, k > 0 the loss's parameter.  No factor math: the losses themselves are applied in K2, on the device."""
from __future__ import annotations

import math

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3          # VF_LOSS_*
NAMES = ("none", "huber", "cauchy", "geman_mcclure")


def loss_id(loss) -> int:
    """id of a loss given by name ("huber"; "geman-mcclure", "gm" and "GemanMcClure" are accepted), by id, or None"""
    if loss is None:
        return NONE
    if isinstance(loss, str):
        key = loss.lower().replace("-", "_").replace(" ", "_")
        key = {"gm": "geman_mcclure", "gemanmcclure": "geman_mcclure"}.get(key, key)
        if key not in NAMES:
            raise ValueError(f"unknown robust loss {loss!r}: one of {NAMES}")
        return NAMES.index(key)
    i = int(loss)
    if not 0 <= i < len(NAMES):
        raise ValueError(f"unknown robust loss id {loss!r}")
    return i


def loss_name(loss) -> str:
    return NAMES[loss_id(loss)]


def parse(robust):
    """(id, k) of the `robust` argument the managers take: None, a name with a default k of 1 standard deviation x the usual
    tuning constant, or (name or id, k)"""
    if robust is None:
        return NONE, 0.0
    if isinstance(robust, (str, int)):
        i = loss_id(robust)
        return i, (0.0 if i == NONE else DEFAULT_K[i])
    loss, k = robust
    i, k = loss_id(loss), float(k)
    if i != NONE and not (k > 0.0 and math.isfinite(k)):
        raise ValueError(f"robust loss parameter k must be finite and > 0, got {k!r}")
    return i, (0.0 if i == NONE else k)


# the 95 % asymptotic-efficiency constants of the literature (GTSAM's documentation quotes the same): a default, not a tuning
DEFAULT_K = {HUBER: 1.345, CAUCHY: 2.3849, GEMAN_MCCLURE: 1.0}


def rho(loss, k, s):
    """the loss of a whitened residual norm s: what a robust factor contributes to the cost"""
    i, s = loss_id(loss), float(s)
    if i == NONE or (i == HUBER and s <= k):
        return 0.5 * s * s
    if i == HUBER:
        return k * (s - 0.5 * k)
    u = (s / k) ** 2
    if i == CAUCHY:
        return 0.5 * k * k * math.log1p(u)
    return 0.5 * s * s / (1.0 + u)


def weight(loss, k, s):
    """rho'(s) / s: the weight GTSAM's reweighting gives the factor, 1 for a Gaussian factor"""
    i, s = loss_id(loss), float(s)
    if i == NONE or (i == HUBER and s <= k):
        return 1.0
    if i == HUBER:
        return k / s
    u = (s / k) ** 2
    return 1.0 / (1.0 + u) if i == CAUCHY else 1.0 / (1.0 + u) ** 2


def norm_from_error(loss, k, e):
    """the whitened residual norm s of a factor whose error (rho(s), as factor_errors reports it) is e: the inverse of rho in
    closed form.  Geman-McClure saturates at k^2 / 2: an error at or beyond it has no finite norm (inf)."""
    i, e = loss_id(loss), float(e)
    if e < 0.0:
        raise ValueError("a factor error is >= 0 (-1 marks a slot without a factor)")
    if i == NONE or (i == HUBER and e <= 0.5 * k * k):
        return math.sqrt(2.0 * e)
    if i == HUBER:
        return e / k + 0.5 * k
    if i == CAUCHY:
        return k * math.sqrt(math.expm1(2.0 * e / (k * k)))
    d = k * k - 2.0 * e
    return k * math.sqrt(2.0 * e / d) if d > 0.0 else math.inf


def weight_from_error(loss, k, e):
    """rho'/s of a factor from its error alone: how far the loss has down-weighted it (1: not at all)"""
    i, e = loss_id(loss), float(e)
    if i == GEMAN_MCCLURE:            # w = 1 / (1 + u)^2 and 2 e / k^2 = u / (1 + u): w = (1 - 2 e / k^2)^2, finite where s is not
        if e < 0.0:
            raise ValueError("a factor error is >= 0 (-1 marks a slot without a factor)")
        return max(0.0, 1.0 - 2.0 * e / (k * k)) ** 2
    if i == CAUCHY:                   # w = 1 / (1 + u), 1 + u = exp(2 e / k^2)
        if e < 0.0:
            raise ValueError("a factor error is >= 0 (-1 marks a slot without a factor)")
        return math.exp(-2.0 * e / (k * k))
    return weight(i, k, norm_from_error(i, k, e))
