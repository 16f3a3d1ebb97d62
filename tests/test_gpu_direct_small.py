"""-m gpu: the INCREMENT of one direct band solve, in every form K4 takes, against the exact least-squares reference of the
window's whitened rows (tests/direct_ref.py on top of tests/refine_ref.py).

Every other test of these forms is a trajectory after LM trials (LM forgives the increment), one device form against another
or against the oracle's band Cholesky of the device's own read_normal (bars of 1e-3 and 1e-4 relative to the LARGEST entry of
the increment, which bias and rotation components cannot fail), or bit equality between forms that share an order (the same,
not right).  Here every window has to satisfy  err(delta, dref) <= 16 x S[case, lambda]  -- err scales every tangent
component by its own size, S is the largest error of three correct float64 evaluations of the same normal equations, fixed on
the CPU by tests/test_direct_ref_host.py, which also shows that normal equations wrong in one between factor, in lambda on one
keyframe, ... land beyond 10 x that bar.  Every case runs at lambda = 1e-5 and at lambda = 1: a wrong damping term is
invisible at the default (direct_ref.LAMBDA_BLIND).

All ladder and offset cases of one lambda are ONE ragged batch per form, one case per window.  Every solve is driven as
tests/test_gpu_refine_small.py drives it: reset_lambda(), linearize(0), decide(init), assemble(), solve(), read_delta, and then
retract(), linearize(1), decide() so that read_lm's solve_failures says whether the solve failed.  Every test asserts
solve_form(): it tests the form it names."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_sharded.py: imported after it, torch.cuda finds no GPU)

from tests import direct_ref as dr
from tests import helpers
from tests import refine_ref as rr

pytestmark = pytest.mark.gpu
_cases, _refs, _runs = {}, {}, {}
ONE_WAVE = dict(chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, solve_split_min=0)
BATCH_CAPACITY = 136            # case B's window ends at keyframe 131 (see load)


@pytest.fixture(scope="module")
def ref(oracle):
    """the CPU reference of (case, lambda), built once (0.1 to 2 s each)"""
    def get(name, lam):
        if name not in _cases:
            _cases[name] = dr.make_case(oracle, name)
        if (name, lam) not in _refs:
            _refs[(name, lam)] = dr.reference(oracle, _cases[name], lam)
        return _refs[(name, lam)]
    return get


def make_engine(windows, capacity, lam, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    return Engine(EngineOpts(windows=windows, capacity=capacity, lambda0=lam, refine_iterations=0, lm_excursion=0, **kw))


def load(eng, w, case, capacity):
    """the case's problem as far as the engine has slots for it (case B's problem has 200 keyframes and its window ends at 131:
    factors outside the range stay in the slots on both sides, up to the capacity)"""
    p, n = case.prob, min(case.prob["n"], capacity)
    sel = p["btw_b"] < n
    cut = dict(p, n=n, states=p["states"][:n], imu=p["imu"][:n], btw_a=p["btw_a"][sel], btw_b=p["btw_b"][sel], btw=p["btw"][sel])
    helpers.load_engine(eng, w, cut, lo=case.lo, hi=case.hi)
    if case.far is not None:
        eng.set_extra_between(w, *case.far)


def solve_once(eng, ranges, lam):
    """one solve of every window: [(increment (n, 15), read_lm after the trial was judged)] for ranges = [(lo, hi)] by window"""
    eng.reset_lambda()
    eng.linearize(0)
    eng.decide(True)
    eng.assemble()
    eng.solve()
    assert all(eng.read_lm(w)["lam"] == lam for w in (0, len(ranges) - 1))
    out = [eng.read_delta(w, lo, hi - lo) for w, (lo, hi) in enumerate(ranges)]
    eng.retract()
    eng.linearize(1)
    eng.decide(False)
    return [(d, eng.read_lm(w)) for w, d in enumerate(out)]


def check(f, what, out):
    name, lam = f["case"].name, f["lam"]
    d, lm = out
    e, b = rr.err(d, f["dref"]), dr.bar(name, lam)
    print(f"case {name}, lambda {lam:g}, {what}: error {e:.3e} = {e / b:.3f} of the bar {b:.2e} (S {dr.S[(name, lam)]:.2e}); {lm['solve_failures']} failed solves")
    assert e <= b, (name, lam, what)
    assert lm["solve_failures"] == 0
    return e


def run_batch(ref, lam, form, **kw):
    """every ladder and offset case as one window each of ONE engine: [(increment, lm)] in the order of direct_ref.BATCH_CASES"""
    key = (lam, tuple(sorted(kw.items())))
    if key not in _runs:
        cases = [ref(name, lam)["case"] for name in dr.BATCH_CASES]
        eng = make_engine(len(cases), BATCH_CAPACITY, lam, **kw)
        assert eng.solve_form() == form
        for w, c in enumerate(cases):
            load(eng, w, c, BATCH_CAPACITY)
        _runs[key] = solve_once(eng, [(c.lo, c.hi) for c in cases], lam)
        eng.close()
    return _runs[key]


def check_batch(ref, lam, what, outs):
    for name, out in zip(dr.BATCH_CASES, outs):
        check(ref(name, lam), what, out)


def same_bits(a, b):
    for (da, _), (db, _) in zip(a, b):
        np.testing.assert_array_equal(da, db)


# ---------------------------------------------------------------- 1. the whole-window sweeps
@pytest.mark.parametrize("lam", dr.LAMBDAS)
def test_one_wave_sweep(ref, lam):
    check_batch(ref, lam, "k_band_solve", run_batch(ref, lam, "one_wave", **ONE_WAVE))


@pytest.mark.parametrize("lam", dr.LAMBDAS)
def test_split_sweep_gives_the_bits_of_the_one_wave_sweep(ref, lam):
    """k_band_forward + k_band_backward (solve_backsub_form 1: two per SIMD) / k_band_backward_1w (2: one per SIMD):
    "same arithmetic, same bits" (include/vilfusion.h, solve_split_min)"""
    one = run_batch(ref, lam, "one_wave", **ONE_WAVE)
    for form in (1, 2):
        out = run_batch(ref, lam, "one_wave_split", **dict(ONE_WAVE, solve_split_min=1, solve_backsub_form=form))
        check_batch(ref, lam, f"split, solve_backsub_form = {form}", out)
        same_bits(out, one)


@pytest.mark.parametrize("lam", dr.LAMBDAS)
def test_assembling_sweeps(ref, lam):
    """k_band_forward_asm and k_band_forward_asm2: H is formed inside the sweep, from the Jacobians K1 / K2 leave, and never
    stored -- this is where that H is held to a reference.  One wave and two waves per window: "the same bits"."""
    outs = []
    for waves in (1, 2):
        outs.append(run_batch(ref, lam, "assembling", **dict(ONE_WAVE, solve_assemble_min=1, solve_assemble_waves=waves)))
        check_batch(ref, lam, f"assembling, {waves} wave(s) per window", outs[-1])
    same_bits(outs[0], outs[1])


@pytest.mark.parametrize("lam", dr.LAMBDAS)
def test_two_sided_sweep(ref, lam):
    """k_band_solve_tw with the library's sweep_two_sided_max: what any chunks = 1 engine of up to 256 windows launches.  At
    n = 2, 3, 4, 5 the two waves meet at once; at lambda = 1 the damping of the meeting point counts"""
    assert {"L2", "L3", "L4", "L5"} <= set(dr.BATCH_CASES)
    check_batch(ref, lam, "k_band_solve_tw", run_batch(ref, lam, "two_sided", chunks=1))


# ---------------------------------------------------------------- 2. the partitioned solve
def chunks_expected(n, chunks):
    """chunks a window of n keyframes is cut into (vf_kernels.hpp chunk_count, restated): at most `chunks` -- for chunks = 0,
    the fitted count, at most sqrt(n) --, and every chunk with 8 pivots or more, multiples of 4, one cut keyframe between two"""
    P = int(np.floor(np.sqrt(n))) if chunks == 0 else chunks
    while P > 1 and (((n - (P - 1)) // P) & ~3) < 8:
        P -= 1
    return max(P, 1)


@pytest.mark.parametrize("chunks", (2, 3, 4, 16, 0))
@pytest.mark.parametrize("lam", dr.LAMBDAS)
def test_partitioned_solve(ref, lam, chunks):
    """K4p.  Windows too short for the engine's chunk count use fewer chunks, down to one: what vf_chunk_geometry says they use
    is what chunk_count's rule gives, and the ladder has the lengths at which it goes to 2, 3 and 4 with the length below each.
    At lambda = 1 the damping of the separators counts"""
    from vil_sensor_fusion_amd.distributed import chunk_geometry
    used = {}
    for name in dr.BATCH_CASES:
        n = ref(name, lam)["case"].n
        used[name] = len(chunk_geometry(n, 96 if chunks == 0 else chunks, chunks == 0))
        assert used[name] == chunks_expected(n, chunks), (name, chunks)
    print(f"chunks = {chunks}: chunks used per case {used}")
    assert set(used.values()) >= set(range(1, min(chunks or 4, 4) + 1))          # the fall-backs are reached, not only named
    outs = run_batch(ref, lam, "partitioned", chunks=chunks)
    for name, out in zip(dr.BATCH_CASES, outs):
        check(ref(name, lam), f"chunks = {chunks} ({used[name]} used)", out)


# ---------------------------------------------------------------- 3. the marginal prior
MARG_FORMS = {
    "one_wave": ONE_WAVE,
    "two_sided": dict(chunks=1),
    "assembling": dict(ONE_WAVE, solve_assemble_min=1),
    "partitioned": dict(chunks=4),
}


def device_marg_case(oracle, name, **kw):
    """a marginal-prior case as the DEVICE makes it (tests/test_gpu_refine_small.py::_device_case_m, refine_iterations = 0): LM
    trials and marginalising slides on the engine, then L, eta, xbar from read_marginal and the states from get_states.
    (engine still loaded, the reference of the case rebuilt from what the device holds)"""
    seed, n = {"M": (rr.M_SEED, rr.M_N), "M12": (dr.M12_SEED, dr.M12_N)}[name]
    from vil_sensor_fusion_amd import synth
    prob = helpers.build_problem(oracle, synth.make_sequence(seed=seed, n_kf=n + rr.M_SLIDES), perturb=0.0)
    eng = make_engine(1, prob["n"] + 8, rr.LAMBDA, **kw)
    helpers.load_engine(eng, 0, prob, lo=0, hi=n)
    for _ in range(rr.M_SLIDES):
        eng.iterate(rr.M_TRIALS)
        eng.slide(marginalize=True)
    mg = eng.read_marginal(0)
    assert mg["on"] == 1 and np.abs(mg["L"][21:27]).max() > 0.0
    case = rr.Case(name, prob, eng.get_states(0, 0, prob["n"]), rr.M_SLIDES, n + rr.M_SLIDES, None,
                   marg=dict(L=mg["L"], eta=mg["eta"], xbar=mg["xbar"]), slides=rr.M_SLIDES)
    return eng, case, dr.reference(oracle, case, rr.LAMBDA)


@pytest.mark.parametrize("form", MARG_FORMS)
@pytest.mark.parametrize("name", dr.MARG_CASES)
def test_marginal_prior(oracle, name, form):
    """no X0 prior, the marginal prior's 27 x 27 block on [lo: 15][lo + 1: pose][lo + 2: pose], L[21:27] alive (two slides)"""
    eng, case, f = device_marg_case(oracle, name, **MARG_FORMS[form])
    assert eng.solve_form() == form
    check(f, form, solve_once(eng, [(case.lo, case.hi)], rr.LAMBDA)[0])
    eng.close()


# ---------------------------------------------------------------- 4. far factors: the Woodbury correction
@pytest.mark.parametrize("name", dr.FAR_CASES)
def test_far_factors_every_form(ref, name):
    """two slots on one keyframe, one far factor ending at the last keyframe.  The column engine (default of a single-window
    engine), the per-column loop (far_batch_columns = 0; any engine of several windows), the dense systems in device memory
    (far_big_forms): "same bits" each (include/vilfusion.h).  The assembling sweep does not take far factors."""
    f = ref(name, rr.LAMBDA)
    case = f["case"]
    cap = case.prob["n"] + 8

    def run(windows=1, **kw):
        eng = make_engine(windows, cap, rr.LAMBDA, chunks=1, **kw)
        assert eng.solve_form() == "two_sided"
        for w in range(windows):
            load(eng, w, case, cap)
        out = solve_once(eng, [(case.lo, case.hi)] * windows, rr.LAMBDA)
        eng.close()
        return out

    a = run()[0]
    check(f, "column engine", a)
    loop = run(far_batch_columns=0)[0]
    check(f, "far_batch_columns = 0", loop)
    np.testing.assert_array_equal(loop[0], a[0])
    for w, two in enumerate(run(windows=2)):
        check(f, f"windows = 2, window {w}", two)
        np.testing.assert_array_equal(two[0], a[0])
    big = run(max_far_factors=16, far_big_forms=1)[0]
    check(f, "max_far_factors = 16, far_big_forms = 1", big)
    np.testing.assert_array_equal(big[0], a[0])


# ---------------------------------------------------------------- 5. a batch past one launch of the two-wave assembling sweep
def asm2_launch_chunk():
    """windows per launch of k_band_forward_asm2, read where the library says it: the constant launch_asm2's loop steps by"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vil_sensor_fusion_amd", "csrc", "kernels")
    with open(os.path.join(csrc, "launch.inc")) as fh:
        step = re.search(r"for \(int w0 = 0; w0 < v\.B; w0 \+= (\w+)\)", fh.read())
    assert step, "launch.inc no longer launches the two-wave sweep in chunks of windows"
    with open(os.path.join(csrc, "k4_band_body.inc")) as fh:
        value = re.search(r"constexpr int %s = (\d+);" % step.group(1), fh.read())
    assert value, step.group(1)
    return int(value.group(1))


def test_batch_past_one_launch_chunk_of_the_two_wave_sweep(ref):
    chunk = asm2_launch_chunk()
    windows = chunk + 6
    f = ref("L9", rr.LAMBDA)
    case = f["case"]
    eng = make_engine(windows, 16, rr.LAMBDA, **dict(ONE_WAVE, solve_assemble_min=1, solve_assemble_waves=2))
    assert eng.solve_form() == "assembling"
    for w in range(windows):
        load(eng, w, case, 16)
    outs = solve_once(eng, [(case.lo, case.hi)] * windows, rr.LAMBDA)
    eng.close()
    for w in (0, chunk - 1, chunk, windows - 1):
        check(f, f"window {w} of {windows} (launch chunk {chunk})", outs[w])
    for w in range(1, windows):
        np.testing.assert_array_equal(outs[w][0], outs[0][0])
        assert outs[w][1]["solve_failures"] == 0
