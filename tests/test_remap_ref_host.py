"""What fixes the numbers of tests/remap_ref.py, on the CPU (no GPU): the mpmath reference does not move with its working
precision, the floor S of three correct float64 evaluations of the rule is the written table, the properties the rule promises
(exactly nominal where nothing is deweighted, continuous across the threshold, independent of the eigenbasis where eigenvalues
repeat) hold for the references and the evaluations, and the bar 16 x S + 64 eps would catch the rule wrong in one place.
tests/test_gpu_remap.py holds the device to the same table."""
import numpy as np
import pytest

from tests import cov_ref as cr
from tests import refine_ref as rr
from tests import remap_ref as mr


def test_tables_name_what_exists():
    assert set(mr.S) == set(mr.CASES) == set(mr.cases()) == set(mr.DEWEIGHTED)
    assert mr.bar("tunnel") == tuple(rr.BAR_FACTOR * s + cr.POSE_ROUNDING for s in mr.S["tunnel"])
    for name in mr.CASES:
        H = mr.cases()[name][0]
        assert np.array_equal(H, H.T) and H.shape == (6, 6)


@pytest.mark.parametrize("name", mr.CASES)
def test_reference_does_not_move_with_its_precision(name):
    """60 digits against 90: the same float64 numbers to within S / 100 (or 2 ulp of rounding the result)"""
    H, tt, rt = mr.cases()[name]
    C, M, E, dw = mr.case_reference(name)
    C2, M2, E2, dw2 = mr.reference(H, mr.NOM6, tt, rt, mr.FLOOR, dps=90)
    e = (mr.err(C2, C), mr.err(M2, M), mr.eig_err(E2, E))
    print(f"case {name}: 60 against 90 digits {e}; deweighted {dw}")
    assert dw == dw2 == mr.DEWEIGHTED[name]
    assert all(x <= max(s / 100.0, 2.0 * cr.EPS) for x, s in zip(e, mr.S[name]))


@pytest.mark.parametrize("name", mr.CASES)
def test_floor_is_the_written_constant(name):
    s, errs = mr.measure(name)
    print(f"case {name}: S measured ({s[0]:.3e}, {s[1]:.3e}, {s[2]:.3e}), written {mr.S[name]}, bar {mr.bar(name)}: " +
          "; ".join(f"{k} {v[0]:.3e} {v[1]:.3e} {v[2]:.3e}" for k, v in errs.items()))
    for measured, written in zip(s, mr.S[name]):
        assert measured <= written <= 1.25 * measured


@pytest.mark.parametrize("name", mr.EXACTLY_NOMINAL)
def test_nothing_deweighted_is_exactly_nominal(name):
    """the additive form gives Sigma = N and G = I to the bit when every g is 1, whatever the eigenvectors' rounding"""
    H, tt, rt = mr.cases()[name]
    C, M, _, dw = mr.case_reference(name)
    assert dw == 0 and np.array_equal(C, np.diag(mr.NOM6))
    for which, (c, m, _) in mr.evaluations(H, mr.NOM6, tt, rt, mr.FLOOR).items():
        if "additive" in which:
            assert c.tobytes() == np.diag(mr.NOM6).tobytes(), which
            s = np.sqrt(mr.NOM6)
            assert np.array_equal(m, np.eye(6) / np.outer(s, s)), which


def test_continuous_across_the_threshold():
    """threshold- differs from threshold+ by what the rule says a relative step of 2e-9 in one eigenvalue does -- the weight
    1 / g - 1 = 1e-9 / (1 - 1e-9) on one direction, at most that much of sqrt(N_ii N_jj) in any entry -- and by no jump: the
    two references are that close, bar added, and so is every evaluation of one to the reference of the other"""
    w = 1e-9 / (1.0 - 1e-9)
    Cp, Mp, _, _ = mr.case_reference("threshold+")
    Cm, Mm, _, _ = mr.case_reference("threshold-")
    bc, bi, _ = mr.bar("threshold-")
    print(f"references: cov {mr.err(Cm, Cp):.3e}, info {mr.err(Mm, Mp):.3e}; the step {w:.3e}")
    assert 0.0 < mr.err(Cm, Cp) <= w + bc and 0.0 < mr.err(Mm, Mp) <= w + bi
    H, tt, rt = mr.cases()["threshold-"]
    for which, (c, m, _) in mr.evaluations(H, mr.NOM6, tt, rt, mr.FLOOR).items():
        assert mr.err(c, Cp) <= w + bc and mr.err(m, Mp) <= w + bi, which


@pytest.mark.parametrize("name", ["two equal", "all equal"])
def test_repeated_eigenvalues_do_not_depend_on_the_eigenbasis(name):
    """Sigma is a spectral function of H': any orthonormal basis of a repeated eigenvalue's space gives the same matrix.  The
    rotated basis is orthonormal to `defect` only (a QR in float64); the sums weigh that by at most 1 / g - 1 against a
    Sigma of at least 1 / g (no amplification) and by 1 - g against an M that may be as small as g_min (1 / g_min), six terms each"""
    H, tt, rt = mr.cases()[name]
    C, M, _, _ = mr.case_reference(name)
    d = mr._d(tt, rt)
    lam, V = np.linalg.eigh(H * np.outer(d, d))
    k = 2 if name == "two equal" else 6                      # the space of the smallest eigenvalue
    assert np.ptp(lam[:k]) <= 1e-12 * np.abs(lam).max()         # equal to the rounding of the eigen-solve, eps ||H'||
    rng = np.random.default_rng(11)
    bc, bi, _ = mr.bar(name)
    for _ in range(4):
        Q = np.linalg.qr(rng.normal(size=(k, k)))[0]
        V2 = V.copy()
        V2[:, :k] = V[:, :k] @ Q
        defect = np.abs(V2.T @ V2 - np.eye(6)).max()
        c, m = mr.additive(np.r_[np.full(k, lam[:k].mean()), lam[k:]], V2, mr.NOM6, mr.FLOOR)
        g_min = max(lam[0], mr.FLOOR)
        print(f"case {name}: rotated basis (defect {defect:.1e}), cov {mr.err(c, C):.3e} (bar {bc:.3e}), info {mr.err(m, M):.3e} (bar {bi:.3e}, 1 / g_min {1 / g_min:.3g})")
        assert mr.err(c, C) <= bc + 6.0 * defect and mr.err(m, M) <= bi + 6.0 * defect / g_min


def test_the_bar_can_fail():
    """every mutation lands beyond 10 x the bar of the covariance in at least one case"""
    seen = {}
    for name in mr.CASES:
        C = mr.case_reference(name)[0]
        for what, Cm in mr.mutations(name).items():
            seen.setdefault(what, {})[name] = mr.err(Cm, C) / mr.bar(name)[0]
    for what, by_case in seen.items():
        visible = sorted(c for c, m in by_case.items() if m > 10.0)
        print(f"{what}: visible in {visible}; blind in {sorted(set(by_case) - set(visible))}; " + ", ".join(f"{c} {m:.3g}" for c, m in by_case.items()))
        assert visible, what
    assert set(seen) == {"thresholds x 2", "floor x 10", "nom6 reversed", "order swapped", "N^1/2 on one side only"}
    assert len([c for c, m in seen["nom6 reversed"].items() if m > 10.0]) == len(mr.CASES)
    assert seen["floor x 10"]["below floor"] > 10.0 and seen["floor x 10"]["tunnel"] < 1.0      # (seen only where a g sits below 10 x floor)


def test_err_sees_what_it_should():
    C = mr.case_reference("tunnel")[0]
    assert mr.err(C, C) == 0.0
    x = C.copy()
    x[0, 3] += 1e-3 * np.sqrt(C[0, 0] * C[3, 3])
    assert abs(mr.err(x, C) - 1e-3) < 1e-12
    R = np.triu(np.arange(1.0, 37.0).reshape(6, 6))
    assert np.array_equal(mr.info_of(R[np.triu_indices(6)]), R.T @ R)
