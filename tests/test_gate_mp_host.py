"""The float64 restatement of the innovation gate (tests/gate_ref.gate_f64, on the CPU oracle) against its extended-precision
reference (gate_ref.gate_mp).  No GPU: this fixes, on the CPU, the bar the device test (tests/test_gpu_gate.py) holds
k_gate_between's nis to, and checks the claim the kernel rests on -- the pose rows of G = -B^-1 A are the first six rows of A.

Cases: the step lists "one step", "60 steps, dt in [1e-4, 2e-2]", "zero dt in the middle" (tests/pim_cases.py) and an empty one,
crossed with a in {i, i-1}, crossed with a consistent measurement (the predicted relative pose moved by 0.3 sigma) and a gross one
(1 m, 0.3 rad), under a covariance that is not diagonal (gate_ref.cov36).  "no steps" with a = i is no case: a factor between a
keyframe and itself (VF_GATE_DEGENERATE).  The keyframes and their joint blocks Sigma_ii, Sigma_{i,i-1}, Sigma_aa come from the dense
inverse of a 6-keyframe oracle window (the oracle's own inverse: an input, not the thing tested); keyframe i's bias is the case's
bias estimate.

Bars:
  * the state and xi: 1e-12 per component (tests/test_propagate_mp_host.STATE_BAR);
  * nis, relative: NIS_BAR = 16 x HOST_WORST, HOST_WORST the worst relative nis error this test measures over the cases.  The
    consistent cases set it: their residual is the difference of two poses tens of metres from the origin taken to 0.3 sigma of a
    centimetre-level noise, so one ulp of the predicted position is 1e-13 of the residual before any arithmetic of the gate's own.
    The factor 16 allows for the device's fma contraction and summation order, as tests/test_propagate_mp_host.py does.

Measured here (CPU oracle, float64): 1.67e-12 ("60 steps", a = i, consistent; the other consistent cases 2.5e-15 .. 1.0e-12, the gross
ones 0 .. 2.9e-15), written down below rounded up to two digits: HOST_WORST = 1.7e-12, hence NIS_BAR = 2.72e-11.  The test checks
that what it measures is that constant (not above it, not below half of it), so the bar is a number on the page and never follows
the code under test."""
import functools

import numpy as np
import pytest

from tests import gate_ref, helpers
from tests.test_propagate_mp_host import STATE_BAR, case_steps
from vil_sensor_fusion_amd import synth

STEP_LISTS = ["one step", "60 steps, dt in [1e-4, 2e-2]", "zero dt in the middle", "no steps"]
CASES = [(s, a, k) for s in STEP_LISTS for a in ("i", "i-1") for k in ("consistent", "gross") if not (s == "no steps" and a == "i")]
HOST_WORST = 1.7e-12
NIS_BAR = 16 * HOST_WORST
GP_BAR = 1e-15      # the Jacobians reach gate_mp rounded to float64 once: entries of size 1, a few ulps


@functools.lru_cache(maxsize=None)
def window():
    """states and dense covariance of a 6-keyframe oracle window after 3 LM trials"""
    from oracle import oracle
    oracle.build()
    seq = synth.make_sequence(seed=21, n_kf=6)
    win = helpers.oracle_window(oracle, helpers.build_problem(oracle, seq, perturb=0.01))
    win.lm(iterations=3)
    _, Hb, _ = win.assemble()
    n = win.n_kf
    H = np.zeros((15 * n, 15 * n))
    for k in range(n):
        for d in range(Hb.shape[1]):
            if k - d >= 0:
                H[15 * k:15 * k + 15, 15 * (k - d):15 * (k - d) + 15] = Hb[k, d]
                H[15 * (k - d):15 * (k - d) + 15, 15 * k:15 * k + 15] = Hb[k, d].T
    s = 1.0 / np.sqrt(np.diag(H))
    S = np.linalg.inv(H * np.outer(s, s)) * np.outer(s, s)
    return np.array(win.states), 0.5 * (S + S.T)


def blocks(a):
    """(x_i, x_a, Sigma_ii, Sigma_{i,a}, Sigma_aa) of the window for a = "i" or "i-1" """
    x, S = window()
    Sii = S[-15:, -15:]
    if a == "i":
        return x[-1].copy(), x[-1].copy(), Sii, Sii, Sii
    return x[-1].copy(), x[-2].copy(), Sii, S[-15:, -30:-15], S[-30:-15, -30:-15]


@functools.lru_cache(maxsize=None)
def measured(steps_name, a, kind):
    from oracle import oracle
    steps, bhat, cov = case_steps(steps_name)
    x_i, x_a, Sii, Sia, Saa = blocks(a)
    x_i[10:16] = bhat
    if a == "i":
        x_a = x_i.copy()
    x_j = gate_ref.predict_f64(oracle, steps, cov, x_i)[0]
    rec = gate_ref.measurement(oracle, x_a, x_j, gate_ref.cov36(), kind)
    ref = gate_ref.gate_mp(steps, cov, x_i, x_a, Sii, Sia, Saa, rec)
    got = gate_ref.gate_f64(oracle, steps, cov, x_i, x_a, Sii, Sia, Saa, rec)
    return dict(n=len(steps), ref=ref, got=got, nis=abs(got["nis"] - ref["nis"]) / ref["nis"],
                nis_m=abs(got["nis_measurement"] - ref["nis_measurement"]) / ref["nis_measurement"],
                xi=float(np.max(np.abs(got["xi"] - ref["xi"]))), state=float(np.max(np.abs(got["state"] - ref["state"]))))


@pytest.mark.parametrize("steps_name,a,kind", CASES)
def test_restatement_against_mpmath(oracle, steps_name, a, kind):
    m = measured(steps_name, a, kind)
    print(f"\n{steps_name:30s} a = {a:3s} {kind:10s}: nis {m['ref']['nis']:.6e} rel. error {m['nis']:.2e} (bar {NIS_BAR:.2e})  "
          f"nis_measurement {m['ref']['nis_measurement']:.4e} ({m['nis_m']:.1e})  xi {m['xi']:.1e}  state {m['state']:.1e}  G_p rows {m['ref']['gp_rows']:.1e}")
    assert np.all(np.linalg.eigvalsh(m["ref"]["S"]) >= 1.0 - 1e-12)       # S = I + a covariance
    assert m["state"] <= STATE_BAR and m["xi"] <= STATE_BAR
    assert m["nis"] <= NIS_BAR
    assert m["ref"]["gp_rows"] <= GP_BAR
    # what the statistic means: a 0.3-sigma move is far inside any threshold, a metre is far outside; the prior never adds information
    assert m["ref"]["nis"] <= m["ref"]["nis_measurement"] * (1 + 1e-12)
    if kind == "consistent":
        assert m["ref"]["nis"] <= 0.09 * 1.0001
    else:
        assert m["ref"]["nis"] > 22.46


def test_the_constant_is_the_measured_one(oracle):
    """HOST_WORST is what this test measures, rounded up: never below the measurement, at most twice it"""
    worst = max(measured(*c)["nis"] for c in CASES)
    print(f"\nworst relative nis error of the float64 restatement {worst:.3e}; HOST_WORST {HOST_WORST:.1e}; NIS_BAR {NIS_BAR:.2e}")
    assert worst <= HOST_WORST <= 2.0 * worst
