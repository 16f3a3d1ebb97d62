"""What fixes the numbers of tests/refine_ref.py, on the CPU (no GPU): the extended-precision least-squares reference has
converged and agrees with an independent solver, the float64 restatement of the refined solve lands where the written
constants say, the bars derived from them would catch an operator that is wrong in one row class, and where refinement
helps.  tests/test_gpu_refine_small.py holds the device to the same constants."""
import numpy as np
import pytest

from tests import refine_ref as rr

CASES = ("A", "B", "F", "M")
_cache = {}


@pytest.fixture(scope="module")
def ref(oracle):
    def get(name):
        if name not in _cache:
            _cache[name] = rr.reference(oracle, rr.make_case(oracle, name))
        return _cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_reference_converged(ref, name):
    f = ref(name)
    print(f"case {name}: {f['rows'].J.shape[0]} rows, {f['rows'].J.shape[1]} columns; corrections of the semi-normal refinement {f['sizes']}")
    assert f["last"] < 1e-15 and len(f["sizes"]) <= 6


def test_cases_reach_what_they_are_for(ref):
    rw = ref("A")["rows"]
    spans = [b[2] - b[1] for b in rw.find("btw")]
    assert [spans.count(s) for s in (1, 2, 3)] == [23, 23, 22] and len(rw.find("prior")) == 1
    b = ref("B")
    assert b["case"].lo % 8 != 0 and b["case"].lo % 64 != 0 and b["case"].prior_k == b["case"].lo
    p = b["case"].prob
    assert np.any(p["btw_a"] < b["case"].lo) and np.any(p["btw_b"] >= b["case"].hi)     # factors outside the range stay in the slots
    far = ref("F")["rows"].find("far")
    assert len(far) == 3 and far[0][1] == far[1][1]                                       # two slots on one keyframe
    m = ref("M")["case"]
    assert m.prior_k is None and np.abs(m.marg["L"][21:27]).max() > 0.0                   # the prior's rows of keyframe lo + 2 are alive


@pytest.mark.parametrize("name", ("A", "B"))
def test_independent_solver_agrees(ref, name):
    """twin_qr.Problem.solve_qr on the same factors: autodiff Jacobians of the twin's own residuals, sequential QR"""
    f = ref(name)
    prob = rr.twin_problem(f["case"])
    d = prob.solve_qr(prob.linearize(), rr.LAMBDA)
    e = rr.err(d, f["dref"])
    print(f"case {name}: solve_qr vs exact {e:.3e}")
    assert e <= 1e-9


def test_far_preconditioner_is_the_inverse_of_the_dense_matrix(oracle, ref):
    """case F: the Woodbury form solves with the dense H + lambda I + U^T U: normwise backward error
    |M x - v| / (|M| |x| + |v|), evaluated in extended precision, for the gradient and for a random right-hand side"""
    f = ref("F")
    msolve, g, H, U = rr.preconditioner(oracle, f["case"], f["rows"])
    M = (rr.band_dense(H) + rr.LAMBDA * np.eye(g.size) + U.T @ U).astype(np.longdouble)
    Mn = float(np.abs(M).sum(axis=1).max())
    for v in (-g, np.random.default_rng(3).normal(size=g.size)):
        x = msolve(v)
        be = float(np.abs(M @ x.astype(np.longdouble) - v).max() / (Mn * np.abs(x).max() + np.abs(v).max()))
        print(f"backward error of the Woodbury solve against the dense matrix: {be:.3e}")
        assert be < 1e-13


@pytest.mark.parametrize("name", CASES)
def test_restatement_error_is_the_written_constant(ref, name):
    f = ref(name)
    e0, e = rr.err(f["res"]["start"], f["dref"]), rr.err(f["res"]["x"], f["dref"])
    print(f"case {name}: start {e0:.3e}, after {f['res']['corrections']} corrections {e:.3e} (written {rr.E_CASE[name]:.2e}, bar {rr.bar(name):.2e}), "
          f"reduction {f['res']['reduction']:.3e}")
    assert e <= rr.E_CASE[name] <= 1.25 * e
    assert 1 <= f["res"]["corrections"] <= rr.REFINE


@pytest.mark.parametrize("name", CASES)
def test_reference_moves_this_much_with_the_rounding_of_its_inputs(ref, name):
    """the same factors linearised by oracle/twin_qr.py, another correct float64 evaluation: U_CASE.  Far below E_CASE in A, B
    and F; in case M, whose increment is tiny, it is what the device's distance from dref consists of"""
    f = ref(name)
    u = rr.input_sensitivity(f["case"], f["rows"], f["dref"])
    print(f"case {name}: twin's rows move dref by {u:.3e} (written {rr.U_CASE[name]:.2e}; restatement {rr.E_CASE[name]:.2e})")
    # (a rounding figure of the twin's autodiff and a LAPACK QR, which moves with the BLAS: the written value may not be
    # undercut by much -- the bar rests on it -- and has to be of the measured order)
    assert 0.1 * rr.U_CASE[name] <= u <= 1.5 * rr.U_CASE[name]
    assert (rr.INPUT_FACTOR * rr.U_CASE[name] < 1e-4 * rr.bar(name)) == (name != "M")


@pytest.mark.parametrize("name", CASES)
def test_the_bar_can_fail(oracle, ref, name):
    """the operator wrong in one row class -- gradient and preconditioner untouched -- lands beyond 10 x the bar: a
    condition on the INPUTS (window, lambda, corrections), which is why the cases are what they are"""
    f = ref(name)
    muts = rr.mutations(f["case"], f["rows"])
    want = {"span-3 between factor without its a block", "span-3 between factor without its rows", "no lambda",
            "bias columns of the last IMU factor dropped"}
    want |= {"marginal prior's rows of keyframe lo + 2 dropped"} if name == "M" else {"X0 prior's rows dropped"}
    want |= {"a block of the last far factor dropped"} if name == "F" else set()
    assert set(muts) == want
    for what, A in muts.items():
        e = rr.err(rr.restatement(oracle, f["case"], f["rows"], A=A)["x"], f["dref"])
        print(f"case {name}, {what}: {e:.3e} = {e / rr.bar(name):.1f} x the bar")
        assert e > 10.0 * rr.bar(name), what


@pytest.mark.parametrize("name", CASES)
def test_where_refinement_must_help(ref, name):
    f = ref(name)
    e0, e = rr.err(f["res"]["start"], f["dref"]), rr.err(f["res"]["x"], f["dref"])
    print(f"case {name}: start / refined = {e0 / e:.1f}")
    assert (e0 >= 8.0 * e) == rr.IMPROVES_8X[name]


def test_stop_rule_separates_the_two_thresholds_on_case_a(oracle, ref):
    """what tests/test_gpu_refine_small.py::test_count_and_stop_rule asks of the device: the first correction of case A leaves a
    reduction between the default threshold (1e-8 squared) and 0.5 squared, so the default goes on and 0.5 stops"""
    f = ref("A")
    full = f["res"]
    early = rr.restatement(oracle, f["case"], f["rows"], rel_stop=0.5)
    print(f"default: {full['corrections']} corrections, reduction {full['reduction']:.3e}; 0.5: {early['corrections']}, {early['reduction']:.3e}")
    assert (early["corrections"], full["corrections"]) == (1, 2)
    assert rr.REL_STOP ** 2 < early["reduction"] <= 0.25 and full["reduction"] <= rr.REL_STOP ** 2


def test_more_corrections_do_not_help(oracle, ref):
    """the CPU finding of DESIGN.md 4a: the float64 restatement is at its floor after ONE correction"""
    for name in CASES:
        f = ref(name)
        e1 = rr.err(rr.restatement(oracle, f["case"], f["rows"], corrections=1)["x"], f["dref"])
        e6 = rr.err(rr.restatement(oracle, f["case"], f["rows"], corrections=6)["x"], f["dref"])
        print(f"case {name}: 1 correction {e1:.3e}, up to 6 {e6:.3e}")
        assert e1 <= 2.0 * rr.E_CASE[name] and e6 >= 0.5 * e1
