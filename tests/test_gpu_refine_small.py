"""-m gpu: the refined solve (csrc/vf_refine.hip: k_jv, k_jtu, k_far_apply, the k_pcg_* steps) at SMALL windows against an
exact least-squares reference of the same linear problem.

Every other test of these kernels is end to end: 1 600 to 10 000 keyframes, and a trajectory that lands within some ATE of
the oracle's -- conjugate gradients behind a good preconditioner forgive an operator that is wrong in one row class, and LM
forgives the increment.  Here refine_iterations = 4 forces the refined solve on windows of 70 to 128 keyframes and the
INCREMENT of one solve is compared with tests/refine_ref.exact: the extended-precision minimiser of the window's whitened
rows.  The bar of a case is 16 x (the error the float64 restatement of the algorithm has against the same reference + how far
that reference moves under another float64 linearisation of its factors): refine_ref.E_CASE and U_CASE, fixed on the CPU by
tests/test_refine_ref_host.py, which also shows that an operator without one between factor's a block, without lambda,
without the prior's rows ... lands beyond 10 x that bar.

Every engine is driven the same way: reset_lambda(), linearize(0), decide(init), assemble(), solve(), read_delta / read_refine, and then
retract(), linearize(1), decide() so that read_lm's solve_failures says whether the solve failed."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_sharded.py: imported after it, torch.cuda finds no GPU)

from tests import helpers
from tests import refine_ref as rr
from vil_sensor_fusion_amd import synth

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def ref(oracle):
    """the CPU reference of a case (built once: 2 to 4 s each)"""
    def get(name):
        if name not in _cache:
            _cache[name] = rr.reference(oracle, rr.make_case(oracle, name))
        return _cache[name]
    return get


def make_engine(windows=1, capacity=78, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    opts = dict(refine_iterations=rr.REFINE, lm_excursion=0, chunks=1)
    opts.update(kw)
    return Engine(EngineOpts(windows=windows, capacity=capacity, **opts))


def load(eng, w, case):
    helpers.load_engine(eng, w, case.prob, lo=case.lo, hi=case.hi)
    if case.far is not None:
        eng.set_extra_between(w, *case.far)


def solve_once(eng, ranges):
    """one solve of every window; [(increment (n, 15), corrections, reduction, lm)] for ranges = [(lo, hi)] by window"""
    eng.reset_lambda()                      # (LM trials before this solve -- case M -- have moved lambda: back to lambda0)
    eng.linearize(0)
    eng.decide(True)
    eng.assemble()
    eng.solve()
    assert all(eng.read_lm(w)["lam"] == rr.LAMBDA for w in range(len(ranges)))
    out = [[eng.read_delta(w, lo, hi - lo) if hi > lo else np.zeros((0, 15)), *eng.read_refine(w)] for w, (lo, hi) in enumerate(ranges)]
    eng.retract()
    eng.linearize(1)
    eng.decide(False)
    return [tuple(o) + (eng.read_lm(w),) for w, o in enumerate(out)]


def run_case(case, **kw):
    eng = make_engine(capacity=case.prob["n"] + 8, **kw)
    load(eng, 0, case)
    out = solve_once(eng, [(case.lo, case.hi)])[0]
    eng.close()
    return out


def check(name, what, f, out, limit=None):
    d, it, red, lm = out
    e = rr.err(d, f["dref"])
    limit = rr.bar(name) if limit is None else limit
    print(f"case {name}, {what}: error {e:.3e} = {e / rr.bar(name):.3f} of the bar {rr.bar(name):.2e} (restatement {rr.E_CASE[name]:.2e}); "
          f"{it} corrections, reduction {red:.3e}, {lm['solve_failures']} failed solves")
    assert e <= limit
    assert 1 <= it <= rr.REFINE and lm["solve_failures"] == 0
    return e


# ---------------------------------------------------------------- 1. the cases against dref
@pytest.mark.parametrize("name", ["A", "B"])
def test_refined_increment_against_exact_least_squares(ref, name):
    f = ref(name)
    e = check(name, "sweeps", f, run_case(f["case"]))
    if rr.IMPROVES_8X[name]:
        e0 = rr.err(run_case(f["case"], refine_iterations=0)[0], f["dref"])
        print(f"case {name}: unrefined {e0:.3e}, refined {e:.3e}")
        assert e <= 0.5 * e0


def _device_case_m(oracle, refine):
    """case M as the DEVICE makes it: LM trials and two marginalising slides on the engine, then L, eta, xbar from
    read_marginal and the states from get_states.  (engine still loaded, the case, its reference)"""
    _, prob = rr.problem(oracle, "M")
    eng = make_engine(capacity=prob["n"] + 8, refine_iterations=refine)
    helpers.load_engine(eng, 0, prob, lo=0, hi=rr.M_N)
    for _ in range(rr.M_SLIDES):
        eng.iterate(rr.M_TRIALS)
        eng.slide(marginalize=True)
    mg = eng.read_marginal(0)
    assert mg["on"] == 1 and np.abs(mg["L"][21:27]).max() > 0.0
    case = rr.Case("M", prob, eng.get_states(0, 0, prob["n"]), rr.M_SLIDES, rr.M_N + rr.M_SLIDES, None,
                   marg=dict(L=mg["L"], eta=mg["eta"], xbar=mg["xbar"]), slides=rr.M_SLIDES)
    return eng, case, rr.reference(oracle, case)


def test_marginal_prior_rows_against_exact_least_squares(oracle):
    """case M: the mp_on branch of k_jtu, no X0 prior.  The reference is rebuilt from what the device holds."""
    eng, case, f = _device_case_m(oracle, rr.REFINE)
    e = check("M", "marginal prior", f, solve_once(eng, [(case.lo, case.hi)])[0])
    eng.close()
    if rr.IMPROVES_8X["M"]:
        eng0, case0, f0 = _device_case_m(oracle, 0)
        e0 = rr.err(solve_once(eng0, [(case0.lo, case0.hi)])[0][0], f0["dref"])
        eng0.close()
        print(f"case M: unrefined {e0:.3e}, refined {e:.3e}")
        assert e <= 0.5 * e0


# ---------------------------------------------------------------- 2. the partitioned solve as preconditioner
def test_partitioned_preconditioner(ref):
    f = ref("B")
    check("B", "chunks = 4", f, run_case(f["case"], chunks=4))


# ---------------------------------------------------------------- 3. far factors
def test_far_factors_every_form(ref):
    """k_far_apply with two slots on one keyframe, the Woodbury solve as preconditioner: the column engine (default of a
    single-window engine), the per-column loop (far_batch_columns = 0; any engine of several windows), the dense systems in
    device memory (far_big_forms)"""
    f = ref("F")
    case = f["case"]
    a = run_case(case)
    check("F", "column engine", f, a)
    loop = run_case(case, far_batch_columns=0)
    check("F", "far_batch_columns = 0", f, loop)
    np.testing.assert_array_equal(loop[0], a[0])              # the per-column loop gives the bits of the column engine
    eng = make_engine(windows=2, capacity=case.prob["n"] + 8)
    for w in range(2):
        load(eng, w, case)
    two = solve_once(eng, [(case.lo, case.hi)] * 2)
    eng.close()
    for w in range(2):
        check("F", f"windows = 2, window {w}", f, two[w])
        np.testing.assert_array_equal(two[w][0], a[0])        # ... also as one of two windows
    big = run_case(case, max_far_factors=16, far_big_forms=1)
    check("F", "max_far_factors = 16, far_big_forms = 1", f, big)
    np.testing.assert_array_equal(big[0], a[0])               # the device-memory form gives the bits of the LDS form


# ---------------------------------------------------------------- 4. a batch
def test_batch_with_a_failed_and_an_empty_window(oracle, ref):
    fa, fb = ref("A"), ref("B")
    ca, cb = fa["case"], fb["case"]
    cap = cb.prob["n"] + 8
    bad_prob = helpers.build_problem(oracle, synth.make_sequence(50, 16))      # (tests/test_gpu_edge_cases.py::test_indeterminate_system_is_flagged)
    bad_prob["states"] = bad_prob["states"].copy()
    bad_prob["states"][5, 4] = np.nan
    singles = []
    for c in (ca, cb):
        e = make_engine(capacity=cap)
        load(e, 0, c)
        singles.append(solve_once(e, [(c.lo, c.hi)])[0])
        e.close()
    eng = make_engine(windows=3, capacity=cap)
    load(eng, 0, ca)
    load(eng, 1, cb)
    helpers.load_engine(eng, 2, bad_prob)
    out = solve_once(eng, [(ca.lo, ca.hi), (cb.lo, cb.hi), (0, 16)])
    eng.close()
    check("A", "window 0 of 3", fa, out[0])
    check("B", "window 1 of 3", fb, out[1])
    for w in range(2):
        np.testing.assert_array_equal(out[w][0], singles[w][0])
        assert out[w][1:3] == singles[w][1:3]
    print(f"window 2 (indeterminate): {out[2][1]} corrections, {out[2][3]['solve_failures']} failed solves")
    assert out[2][3]["solve_failures"] == 1 and out[2][1] == 0
    # ... and with window 2 empty (hi == lo)
    eng = make_engine(windows=3, capacity=cap)
    load(eng, 0, ca)
    load(eng, 1, cb)
    helpers.load_engine(eng, 2, bad_prob, lo=4, hi=4)
    emp = solve_once(eng, [(ca.lo, ca.hi), (cb.lo, cb.hi), (4, 4)])
    eng.close()
    for w in range(2):
        np.testing.assert_array_equal(emp[w][0], singles[w][0])
        assert emp[w][1:3] == singles[w][1:3] and emp[w][3]["solve_failures"] == 0
    assert emp[2][1] == 0 and emp[2][3]["solve_failures"] == 0


# ---------------------------------------------------------------- 5. count and stop rule
def test_count_and_stop_rule(ref):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    f = ref("A")
    one = run_case(f["case"], refine_iterations=1)
    check("A", "refine_iterations = 1", f, one)
    assert one[1] == 1
    full = run_case(f["case"])
    early = run_case(f["case"], refine_rel_stop=0.5)
    print(f"refine_rel_stop default: {full[1]} corrections, reduction {full[2]:.3e}; 0.5: {early[1]} corrections, reduction {early[2]:.3e}")
    # The rule is tested from the second correction on.  The float64 restatement of case A (tests/test_refine_ref_host.py)
    # reaches a reduction of 1.35e-15 with its first correction: above the default's 1e-16, so the default applies a second
    # one; below 0.25, so refine_rel_stop = 0.5 stops there.  An engine that ignored the option would give equal counts.
    assert 1 <= early[1] < full[1] <= rr.REFINE and early[2] <= 0.25
    eng = Engine(EngineOpts(windows=1, capacity=78, refine_iterations=0, chunks=1))
    assert eng.refine_count() == 0
    eng.close()
    eng = make_engine()
    assert eng.refine_count() == rr.REFINE
    eng.close()


# ---------------------------------------------------------------- 6. the staged path of time-sharded windows
def test_staged_refinement_on_two_shards(ref):
    """case B, four chunks, on two lock-step shards of one process (distributed.LockstepGroup, as tests/test_gpu_sharded.py):
    refine_begin, then { solve_local, all-gather, solve_global, all-reduce, refine_step } x 4, refine_end"""
    from vil_sensor_fusion_amd import distributed as D
    f = ref("B")
    case = f["case"]
    engines = []
    for r in range(2):
        e = make_engine(capacity=case.prob["n"] + 8, chunks=4)
        load(e, 0, case)
        engines.append(e)
    group = D.LockstepGroup(engines, "cuda:0")
    group.begin()                                   # reset_lambda, linearize(0), decide(init) on every shard
    group.solve()                                   # the staged solve, its refinement included
    torch.cuda.synchronize()
    assert group.collectives == 2 * (1 + rr.REFINE)
    outs = [[e.read_delta(0, case.lo, case.n), *e.read_refine(0)] for e in engines]
    group.finish()                                  # retract, linearize(1), decide
    torch.cuda.synchronize()
    outs = [tuple(o) + (e.read_lm(0),) for o, e in zip(outs, engines)]
    for e in engines:
        e.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    assert outs[0][1:3] == outs[1][1:3]
    check("B", "two shards, chunks = 4", f, outs[0])
