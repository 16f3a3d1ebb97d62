"""-m gpu: the marginal covariances of SHORT windows against an exact inverse of the window's own normal equations
(tests/cov_ref.py on top of tests/refine_ref.py and tests/direct_ref.py).

tests/test_gpu_marginals.py and tests/test_gpu_marginals_far.py hold Sigma to cond(H) x eps -- about 1e-4 at their 120 to 200
keyframes -- mostly against an inverse of the device's own H, at windows of 37 keyframes and more.  Here every window has to
satisfy  err(Sigma, Sigma_ref) <= 16 x S[case]  over every block Sigma_kk and Sigma_{k+1,k}: Sigma_ref the extended-precision
inverse of J^T J + L built from the whitened rows of the LOADED states, S the largest error of three correct float64
evaluations of that inverse, fixed on the CPU by tests/test_cov_ref_host.py, which also shows that normal equations wrong in
one between factor, in the damping, in the rows of a keyframe outside the range ... land beyond 10 x that bar.  The windows are
the lengths k_band_selinv treats specially (1 to 4 keyframes: shorter than the 27-row profile), the tile and checkpoint edges,
and ranges with lo != 0 inside longer loaded slots.

All ladder and offset cases are ONE ragged batch per factoring (SolvePlan::factor: split, asm1, asm2), one case per window.  No
LM trial runs before marginals(): the states read back are the bits that were loaded, and Sigma_ref is of them.  A window whose
factorisation failed makes read_marginals raise (VF_ERR_NOT_SPD): every read here is also the check that the flag is clear."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_direct_small.py)

from tests import cov_ref as cr
from tests import refine_ref as rr
from tests.test_gpu_direct_small import BATCH_CAPACITY, ONE_WAVE, device_marg_case, load, make_engine

pytestmark = pytest.mark.gpu
_refs, _runs = {}, {}

# {SolvePlan::factor: (engine options, solve_form() of such an engine)}
FACTORINGS = {
    "split": (dict(ONE_WAVE, solve_split_min=1), "one_wave_split"),
    "asm1": (dict(ONE_WAVE, solve_assemble_min=1, solve_assemble_waves=1), "assembling"),
    "asm2": (dict(ONE_WAVE, solve_assemble_min=1, solve_assemble_waves=2), "assembling"),
}
# engines whose SOLVES take another form and whose marginals factor with `split` all the same (vf_solve_plan.hpp)
SPLIT_ALL_THE_SAME = {"two_sided": dict(chunks=1), "partitioned": dict(chunks=4)}


@pytest.fixture(scope="module")
def ref(oracle):
    """the CPU reference of a case, built once (0.1 to 1.5 s each)"""
    def get(name):
        if name not in _refs:
            _refs[name] = cr.reference(oracle, cr.make_case(oracle, name))
        return _refs[name]
    return get


def read(eng, w, case, pose=False):
    """(cov, cross) of the window -- and the records with pose=True -- after asserting that its states are the loaded bits"""
    n = min(case.prob["n"], BATCH_CAPACITY)
    np.testing.assert_array_equal(eng.get_states(w, 0, n), case.states[:n])
    out = eng.read_marginals(w, case.lo, case.n, cross=True)
    return out + eng.read_pose_marginals(w, case.lo, case.n)[:2] if pose else out


def check(f, what, out):
    name = f["case"].name
    e, b = cr.err(out[0], out[1], f["Sref"]), cr.bar(name)
    print(f"case {name}, {what}: error {e:.3e} = {e / b:.3f} of the bar {b:.2e} (S {cr.S[name]:.2e})")
    assert e <= b, (name, what)
    return e


def run_batch(ref, form, pose=False, **kw):
    """every ladder and offset case as one window each of ONE engine: [(cov, cross, ...)] in the order of cov_ref.BATCH_CASES"""
    key = (pose, tuple(sorted(kw.items())))
    if key not in _runs:
        cases = [ref(name)["case"] for name in cr.BATCH_CASES]
        eng = make_engine(len(cases), BATCH_CAPACITY, rr.LAMBDA, **kw)
        assert eng.solve_form() == form
        for w, c in enumerate(cases):
            load(eng, w, c, BATCH_CAPACITY)
        eng.marginals(pose=pose)
        _runs[key] = [read(eng, w, c, pose) for w, c in enumerate(cases)]
        eng.close()
    return _runs[key]


def same_bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x[0], y[0])
        np.testing.assert_array_equal(x[1], y[1])


# ---------------------------------------------------------------- 1. the three factorings
@pytest.mark.parametrize("factor", FACTORINGS)
def test_every_factoring(ref, factor):
    """split: K3 and k_band_forward.  asm1, asm2: k_band_forward_asm and k_band_forward_asm2 under vf::undamped_whole -- H is
    formed inside the sweep and never stored, so there is no read_normal to compare with: this is where it is held to a reference"""
    kw, form = FACTORINGS[factor]
    assert {"L1", "L2", "L3", "L4", "P3", "P13"} <= set(cr.BATCH_CASES)
    for name, out in zip(cr.BATCH_CASES, run_batch(ref, form, **kw)):
        check(ref(name), f"factor = {factor}", out)


def test_factorings_that_share_an_order_give_the_same_bits(ref):
    """engines whose solves are two-sided or partitioned factor their marginals with `split`: the bits of the split engine.
    One and two waves per window of the assembling sweep: each other's bits"""
    split = run_batch(ref, FACTORINGS["split"][1], **FACTORINGS["split"][0])
    for form, kw in SPLIT_ALL_THE_SAME.items():
        same_bits(run_batch(ref, form, **kw), split)
    same_bits(run_batch(ref, "assembling", **FACTORINGS["asm1"][0]), run_batch(ref, "assembling", **FACTORINGS["asm2"][0]))


# ---------------------------------------------------------------- 2. the marginal prior
@pytest.mark.parametrize("factor", ("split", "asm1"))
def test_marginal_prior(oracle, factor):
    """M12 as the DEVICE makes it (LM trials and two marginalising slides on the engine; no X0 prior, L[21:27] alive).  The states
    are read after the slides and the reference is rebuilt from read_marginal: nothing runs between that read and marginals()"""
    kw, form = FACTORINGS[factor]
    eng, case, _ = device_marg_case(oracle, "M12", **kw)
    assert eng.solve_form() == form
    f = cr.reference(oracle, case)
    assert f["last"] <= cr.S["M12"] / 100.0
    eng.marginals()
    np.testing.assert_array_equal(eng.get_states(0, 0, case.prob["n"]), case.states)
    check(f, f"device-made marginal prior, factor = {factor}", eng.read_marginals(0, case.lo, case.n, cross=True))
    eng.close()


# ---------------------------------------------------------------- 3. far factors: the downdate
def test_far_factors(oracle, ref):
    """marginals(far=True): Sigma = A^-1 - Z C^-1 Z^T (k4_selinv_far.inc) in the LDS form and, with max_far_factors = 16 and
    far_big_forms = 1, in the device-memory form: the same bits, both within the bar.  G17's far factors shrink the covariance
    by rho >= 1.01 (F17's by 1.004): a downdate that is left out or wrong in one factor lands 1e6 x beyond the bar and more.
    The third window, L17, holds no far factor and keeps the bits of the band-only call on an engine without any"""
    names = cr.FAR_CASES + ("L17",)
    cases = [ref(name)["case"] for name in names]
    cap = 17 + 8

    def run(far, with_far=True, **kw):
        eng = make_engine(len(cases), cap, rr.LAMBDA, **kw)
        for w, c in enumerate(cases):
            load(eng, w, c if with_far else ref("L17")["case"], cap)       # (F17, G17 and L17 are one problem: seed 7, 17 keyframes)
        eng.marginals(far=far)
        out = [read(eng, w, c) for w, c in enumerate(cases)]
        eng.close()
        return out

    lds = run(True)
    big = run(True, max_far_factors=16, far_big_forms=1)
    for name, a, b in zip(names, lds, big):
        f = ref(name)
        rho = cr.rho(oracle, f["rows"])
        print(f"case {name}: rho = max (A^-1)_ii / Sigma_ii = {rho:.4f}")
        assert rho >= 1.01 or name != "G17"
        check(f, "far = True, the LDS form", a)
        check(f, "far = True, max_far_factors = 16, far_big_forms = 1", b)
    same_bits(lds, big)
    for a in ref("F17")["case"].states, ref("G17")["case"].states:
        np.testing.assert_array_equal(a, ref("L17")["case"].states)
    band = run(False, with_far=False)
    same_bits(lds[2:], band[2:])
    assert not np.array_equal(lds[0][0], band[0][0]) and not np.array_equal(lds[1][0], band[1][0])


# ---------------------------------------------------------------- 4. the nav_msgs records
def test_pose_records(ref):
    """marginals(pose=True) on the split batch: cov36 and info36 (kernels/kpose.inc) against covariance.ros_pose_covariance of
    Sigma_ref,kk and its inverse, in the norms of tests/test_gpu_pose_marginals.py (cov_ref.pose_err).

    cov36 = R Sigma_pose R^T: its distance from the reference's record is R (Sigma - Sigma_ref) R^T, at most the Sigma bar of
    the case in err's norm, plus the rounding of the two 3 x 3 products and of R, for which that test allows 64 eps:
    bar + 64 eps.  info36 = cov36^-1: to first order its distance is I (cov36 - ref) I, which in the norm of sqrt(I_ii I_jj)
    is the relative distance of cov36 times the condition number cond_s of the diagonally scaled record: cond_s x (bar + 64 eps)
    (cond_s of the REFERENCE's record; pose_err divides by it).  The constants a worst case would add (a rotation can spread an
    entrywise error over a group, up to 9 x) are not in these bars: tests/test_cov_ref_host.py measures that three float64
    evaluations of Sigma stay within S and cond_s x S in these norms, so 16 x S bounds a correct evaluation here as it does
    in err's.  Nothing comes from a device result."""
    kw, form = FACTORINGS["split"]
    plain = run_batch(ref, form, **kw)
    outs = run_batch(ref, form, pose=True, **kw)
    same_bits(outs, plain)                                     # the flag changes nothing of Sigma
    for name, (_, _, cov36, info36) in zip(cr.BATCH_CASES, outs):
        f = ref(name)
        c = f["case"]
        e_cov, e_info = cr.pose_err(cov36, info36, c.states[c.lo:c.hi], f["Sref"])
        b = cr.bar(name) + cr.POSE_ROUNDING
        print(f"case {name}, pose records: cov36 error {e_cov:.3e} = {e_cov / b:.3f} of the bar {b:.2e}; info36 error / cond_s {e_info:.3e} = "
              f"{e_info / b:.3f} of the bar (S {cr.S[name]:.2e})")
        assert np.array_equal(cov36, cov36.transpose(0, 2, 1)) and np.array_equal(info36, info36.transpose(0, 2, 1))
        assert e_cov <= b and e_info <= b, name
