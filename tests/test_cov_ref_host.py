"""What fixes the numbers of tests/cov_ref.py, on the CPU (no GPU): the extended-precision Sigma_ref has converged on every
case to S / 100 or better and does not depend on where its refinement started, the floor S of three correct float64
evaluations of Sigma is the written table, and the bar 16 x S would catch normal equations that are wrong in one row class --
or, where it would not, the tables of cov_ref say so.  tests/test_gpu_marginals_small.py holds the device to the same table."""
import numpy as np
import pytest

from tests import cov_ref as cr
from tests import refine_ref as rr

_refs = {}
TWO_STARTS = ("L4", "L17", "M12", "G17", "P13")          # cases whose reference is built a second time from the other start


@pytest.fixture(scope="module")
def ref(oracle):
    """the CPU reference of a case, built once (0.1 to 1.5 s each)"""
    def get(name):
        if name not in _refs:
            _refs[name] = cr.reference(oracle, cr.make_case(oracle, name))
        return _refs[name]
    return get


def test_cases_reach_what_they_are_for(oracle, ref):
    assert set(cr.S) == set(cr.CASES) and set(cr.LAMBDA_SEEN) == set(cr.CASES)
    one = ref("L1")
    assert one["case"].n == 1 and [b[0] for b in one["rows"].blocks] == ["prior"]           # only the X0 prior
    assert {ref(c)["case"].n for c in cr.LADDER_CASES} >= {1, 2, 3, 4}                       # shorter than the 27-row profile
    for name, (loaded, lo, hi) in cr.OFFSETS.items():
        c = ref(name)["case"]
        assert (c.lo, c.hi, c.prob["n"]) == (lo, hi, loaded) and c.n <= 35 and lo % 8 != 0 and hi < loaded and c.prior_k == lo
        a, b = c.prob["btw_a"], c.prob["btw_b"]
        assert np.any((a < lo) & (b >= lo)) and np.any((a < hi) & (b >= hi))                # between factors reach outside on both sides
    m = ref("M12")["case"]
    assert m.prior_k is None and m.n == 12 and np.abs(m.marg["L"][21:27]).max() > 0.0
    rho = {}
    for name in cr.FAR_CASES:
        far = ref(name)["rows"].find("far")
        assert len(far) == 3 and far[0][1] == far[1][1] and far[2][2] == 16                 # two slots on one keyframe, one ends at the last
        rho[name] = cr.rho(oracle, ref(name)["rows"])
    print(f"rho = max (A^-1)_ii / Sigma_ii: {rho}")
    assert rho["G17"] >= 1.01 and rho["F17"] > 1.0                                           # G17's far factors visibly shrink the covariance


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_converged(ref, name):
    """the last correction of exact_cov is at most S / 100, normalised as the error is"""
    f = ref(name)
    print(f"case {name}: {f['rows'].J.shape[0]} rows, {f['rows'].J.shape[1]} columns; corrections of the refinement {f['sizes']}; "
          f"S / last = {cr.S[name] / f['last']:.0f}")
    assert f["last"] <= cr.S[name] / 100.0 and len(f["sizes"]) <= 6


@pytest.mark.parametrize("name", TWO_STARTS)
def test_two_constructions_of_the_reference_agree(oracle, ref, name):
    """from Householder QR of the rows and from the float64 inverse of the diagonally scaled matrix: within S / 100"""
    f = ref(name)
    other, last, sizes = cr.exact_cov(f["rows"], start="inv")
    e = cr.err_dense(other, f["Sref"])
    print(f"case {name}: start = inv, corrections {sizes}; distance from the start = qr reference {e:.3e} = S / {cr.S[name] / max(e, 1e-300):.0f}")
    assert last <= cr.S[name] / 100.0 and e <= cr.S[name] / 100.0
    assert sizes[0] > 10.0 * f["sizes"][0] or name == "L4"        # (the two starts really differ: this one begins further away)


@pytest.mark.parametrize("name", cr.CASES)
def test_floor_is_the_written_constant(ref, name):
    f = ref(name)
    print(f"case {name}: S measured {f['S']:.3e} (written {cr.S[name]:.2e}, bar {cr.bar(name):.2e}): " + ", ".join(f"{k} {v:.3e}" for k, v in f["errs"].items()))
    assert f["S"] <= cr.S[name] <= 1.25 * f["S"]


@pytest.mark.parametrize("name", cr.BATCH_CASES)
def test_pose_records_need_no_floor_of_their_own(ref, name):
    """The nav_msgs records are R Sigma_pose R^T and its inverse.  In the worst case a rotation spreads an entrywise error over
    a 3 x 3 group (a factor of up to 9 with the group's largest diagonal entry as the scale) and an inverse multiplies it by
    more than cond_s; the bar tests/test_gpu_marginals_small.py sets takes neither constant.  What justifies that is measured
    here: the records of the three float64 evaluations of Sigma, made in plain numpy, stay within the case's S of the
    reference's (cov36) and within cond_s x S (info36), 64 eps of rounding aside: cov_ref.pose_err's norms are no weaker
    than err's."""
    f = ref(name)
    for which, (e_cov, e_info) in f["pose_errs"].items():
        print(f"case {name}, {which}: cov36 {e_cov:.3e}, info36 / cond_s {e_info:.3e} (S {cr.S[name]:.2e})")
        assert e_cov <= cr.S[name] + cr.POSE_ROUNDING and e_info <= cr.S[name] + cr.POSE_ROUNDING


@pytest.mark.parametrize("name", cr.CASES)
def test_the_bar_can_fail(oracle, ref, name):
    """every mutation of cov_ref.mutations lands beyond 10 x the bar: a condition on the INPUTS.  Between factors: all that do
    not touch the X0 prior's keyframe, but for cov_ref.LEFT_OUT (at most one per case).  The rest: but for cov_ref.BLIND, whose
    entries are held to what they record."""
    f = ref(name)
    case, b = f["case"], cr.bar(name)
    muts = cr.mutations(oracle, case, f["rows"])
    kinds = {what for what, _, _ in muts}
    want = {"lambda = 1e-5 left in"}
    prior = 0 if case.prior_k is not None else None
    tested = {fac for _, fac, _ in muts if fac is not None}
    assert tested == {(a, b_) for _, a, b_, _, _ in f["rows"].find("btw") if prior not in (a, b_)}
    assert tested or case.n <= 3                 # (n <= 2 has no between factor, n = 3 none off the X0 prior's keyframe)
    if tested:
        want |= {"between factor's cross block dropped from H", "between factor dropped from H"}
    if case.n > 1:
        want |= {"bias columns of the last IMU factor dropped", "bias columns of the last IMU factor's first keyframe dropped"}
    want |= {"marginal prior's rows of keyframe lo + 2 dropped"} if case.marg is not None else {"X0 prior's rows dropped"}
    want |= {"one far factor left out of the downdate", "the downdate omitted"} if case.far is not None else set()
    want |= {"rows of keyframe hi let in"} if name in cr.OFFSETS or name == "L1" else set()
    assert kinds == want
    weakest, weak = {}, {}
    for what, fac, Sigma in muts:
        m = cr.multiple(Sigma, f["Sref"], b)
        if fac is None:
            print(f"case {name}, {what}: {m:.3g} x the bar" + (" (BLIND)" if (name, what) in cr.BLIND else ""))
            if what == "lambda = 1e-5 left in":
                assert cr.LAMBDA_SEEN[name] <= m <= 1.25 * cr.LAMBDA_SEEN[name]
                assert (m > 10.0) == ((name, what) not in cr.BLIND)
            if (name, what) in cr.BLIND:
                assert m <= cr.BLIND[(name, what)] <= 1.25 * m and cr.BLIND[(name, what)] <= 10.0, what
            else:
                assert m > 10.0, what
        else:
            weakest[what] = min(weakest.get(what, (np.inf, None)), (m, fac))
            if not m > 10.0:
                weak.setdefault(fac, []).append((what, m))
    for what, (m, fac) in weakest.items():
        print(f"case {name}, {what}: {len(tested)} factors, the weakest {fac} at {m:.3g} x the bar")
    for fac, w in weak.items():
        print(f"case {name}, NOT beyond 10 x the bar, factor {fac}: " + ", ".join(f"{what} {m:.3g}" for what, m in w))
    assert set(weak) <= ({cr.LEFT_OUT[name]} if name in cr.LEFT_OUT else set()), weak


def test_tables_name_what_exists():
    assert all(isinstance(f, tuple) and len(f) == 2 and isinstance(f[0], int) for f in cr.LEFT_OUT.values())
    assert set(cr.LEFT_OUT) <= set(cr.CASES) and {c for c, _ in cr.BLIND} <= set(cr.CASES)
    assert cr.bar("L17") == rr.BAR_FACTOR * cr.S["L17"]
    seen = {c for c, m in cr.LAMBDA_SEEN.items() if m > 10.0}
    print(f"lambda = 1e-5 left in is visible in {sorted(seen)}, blind in {sorted(set(cr.CASES) - seen)}")
    assert len(seen) >= len(cr.CASES) - 3                 # the check is carried by almost every case


def test_err_sees_what_it_should():
    """err is 0 on the reference's own blocks, sees one entry of one cross block, and refuses a last cross block that is not zero"""
    rng = np.random.default_rng(0)
    G = rng.normal(size=(45, 45))
    Sref = G @ G.T + 45 * np.eye(45)
    cov, cross = cr.blocks(Sref)
    assert cr.err(cov, cross, Sref) == 0.0
    x = cross.copy()
    x[1, 14, 0] += 1e-3 * np.sqrt(Sref[44, 44] * Sref[15, 15])
    assert abs(cr.err(cov, x, Sref) - 1e-3) < 1e-12
    x = cross.copy()
    x[2, 0, 0] = 1e-300
    with pytest.raises(AssertionError):
        cr.err(cov, x, Sref)
