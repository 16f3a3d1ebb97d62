"""The CPU oracle's preintegration (vfo_pim_integrate / vfo_pim_to_record) against the 50-digit reference of the whole K0
record (tests/mp_pim.py) on every case of tests/pim_cases.py.  The device tests (test_gpu_k0_mp.py) use this oracle's
bars, so it has to be exact first.

Bars, each a constant times the float64 rounding the recursion can accumulate:
  * dt_ij: one rounding per addition, relative n eps;
  * the mean: 8 eps of max |mean| per step (test_gpu_lie_edges' bar);
  * H, row-scaled, and P, scaled by sqrt(P_ii P_jj) of the reference: C_HP n eps;
  * |R P_ref R^T - I| and R's row-scaled entries: C_R eps cond(D P D), D = diag(P)^-1/2: R is chol_upper(P^-1), and a
    relative perturbation of P moves it by up to cond times as much.
At dt = 0 the oracle takes the limit of GTSAM's (1/dt) vHb (.) vHb^T, zero, where 4.0.x itself gives NaN."""
import numpy as np
import pytest

from tests import mp_pim, pim_cases

EPS = mp_pim.EPS
C_HP = 64
C_R = 16
NAMES = [c[0] for c in pim_cases.cases()]


def oracle_record(oracle, steps, bhat, cov):
    prm = oracle.make_imu_params(cov["acc"], cov["gyro"], cov["integration"], cov["bias_acc"], cov["bias_omega"],
                                 cov["bias_acc_omega_int"])
    p = oracle.pim_new(bhat)
    for s in steps:
        oracle.pim_integrate(p, prm, s[1:4], s[4:7], s[0])
    return oracle.pim_fields(p), oracle.pim_to_record(p)


def bars(n, cond):
    return dict(dt=n * EPS, mean=8 * EPS * n, H=C_HP * n * EPS, P=C_HP * n * EPS, whiten=C_R * EPS * cond,
                R=C_R * EPS * cond)


def test_oracle_record_against_mpmath(oracle):
    rows, failed = [], []
    for name, steps, bhat, cov in pim_cases.cases():
        ref = mp_pim.reference(name)
        f, rec = oracle_record(oracle, steps, bhat, cov)
        assert np.all(np.isfinite(rec)) and np.all(np.isfinite(f["cov"])), name
        e = mp_pim.errors(ref, rec[0], rec[1:10], rec[16:70].reshape(9, 6), oracle.unpack_upper(rec[70:], 15), f["cov"])
        b = bars(len(steps), ref["cond"])
        np.testing.assert_array_equal(rec[10:16], bhat)
        rows.append((name, len(steps), ref["cond"], e, b))
        failed += [(name, k, e[k], b[k]) for k in b if not e[k] <= b[k]]
    print(f"\n{'case':34s} {'n':>5s} {'cond':>8s} | {'dt':>8s} {'mean':>8s} {'H':>8s} {'P':>8s} {'whiten':>8s} {'R':>8s}"
          "   (error / bar)")
    for name, n, cond, e, b in rows:
        print(f"{name:34s} {n:5d} {cond:8.1e} | " + " ".join(f"{e[k]:8.1e}" for k in b) + "   "
              + " ".join(f"{e[k] / b[k]:.2f}" for k in b))
    assert not failed, failed


def test_oracle_record_matches_mpmath_at_zero_dt(oracle):
    """a zero-dt step (two IMU samples with one timestamp) is an exact no-op in the oracle, as in the reference: the record
    is bit for bit that of the same steps without it, and finite"""
    for name in ("zero dt first", "zero dt in the middle"):
        _, steps, bhat, cov = pim_cases.case(name)
        assert (steps[:, 0] == 0).sum() == 1
        f, rec = oracle_record(oracle, steps, bhat, cov)
        f0, rec0 = oracle_record(oracle, steps[steps[:, 0] != 0], bhat, cov)
        assert np.all(np.isfinite(rec))
        np.testing.assert_array_equal(rec, rec0)
        np.testing.assert_array_equal(f["cov"], f0["cov"])


def test_reference_self_check():
    """the reference's own H recursion and its total derivative of the mean agree (mp_pim.reference raises otherwise), and
    the reference is internally consistent in float64: R upper with a positive diagonal, R^T R P = I"""
    for name in NAMES:
        ref = mp_pim.reference(name)
        assert ref["h_self"] < mp_pim.H_SELF_CHECK
        R = ref["R"]
        assert np.all(np.tril(R, -1) == 0) and np.all(np.diag(R) > 0)
        assert np.abs(R.T @ R @ ref["P"] - np.eye(15)).max() < 16 * EPS * ref["cond"] * 15, name


@pytest.mark.parametrize("name", ["one axis to 2 pi - 1e-3", "wobbling axis past 2 pi"])
def test_cases_reach_their_angles(name):
    """the large-angle cases do what their names say: theta ends within 1e-3 of 2 pi, or the unwrapped norm passes it"""
    th = np.linalg.norm(mp_pim.reference(name)["mean"][:3])
    assert (th > 2 * np.pi) if "past" in name else (2 * np.pi - 2e-3 < th < 2 * np.pi), th
