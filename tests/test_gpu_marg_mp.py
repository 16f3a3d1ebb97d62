"""-m gpu: k_marginalize entry by entry against the extended-precision reference of tests/mp_marg.py, within the bound derived
there (c 2^-53 B; nothing here is fitted to the device's output).  Every case is load, linearize(0), marginalize(),
read_marginal on a synchronous engine of a handful of short windows; the linearisations the reference starts from are read
back from the device (Engine.read_imu_lin / read_between_lin), the anchor prior's rows -- which have no reader -- come from
mp_lie.prior_factor with their rounding counted as input uncertainty.  tests/test_marg_mp_host.py runs the same cases
through a float64 twin and the C oracle; every test prints its worst |err| / (c 2^-53 B)."""
import numpy as np
import pytest

from tests import helpers
from tests import marg_cases as mc
from tests import mp_marg
from vil_sensor_fusion_amd import Engine, EngineOpts, VilFusionError

pytestmark = pytest.mark.gpu
CAP = 128


@pytest.fixture(scope="module")
def prob(oracle):
    return mc.base_problem(oracle)


def _load(eng, w, prob, lo, n, states, placed, prior_rec):
    """window w = keyframes [lo, lo + n) of the sequence with `states` written over lo .., the between factors `placed`
    ([(first keyframe, [(d, record)])]) and the anchor prior on lo"""
    p = mc.with_spans(prob, placed)
    p["states"] = prob["states"].copy()
    p["states"][lo:lo + len(states)] = states
    p["prior"] = prior_rec
    helpers.load_engine(eng, w, p, lo=lo, hi=lo + n)


def _within(name, got, case, floor_p=0.0):
    """asserts the device's (L, eta) within the bound of the case's reference; returns (reference, lift, ext)"""
    ref = mp_marg.reference(case)
    lift = ext = None
    if floor_p > 0.0:
        Q = mp_marg.gauge_basis(case.states[1:4], case.gravity)
        lift, ext, ev, dMF = mp_marg.floor_lift(ref, Q, floor_p)
        print(f"{name}: gauge eigenvalues of the reference {[float(e) for e in ev]}, floor_p {floor_p:.3e}, |dM|_F {float(dMF):.3e}: "
              + ("above the floor, no lift admissible" if lift is None else "the floor engages"))
    rl, re_ = mp_marg.check(name, got["L"], got["eta"], ref, what="device ", lift=lift, ext=ext)
    assert got["on"] == 1
    assert rl <= 1.0 and re_ <= 1.0, (name, rl, re_)
    return ref, lift, ext


def test_span_patterns_and_placement(oracle, prob):
    """All eight subsets of {span 1, 2, 3} between factors at the leaving keyframe, one per window of one engine; first slots
    6, 7, 62, 63, 64 (both sides of a J-stream tile and of an AoSoA tile), windows of exactly 4 and 5 keyframes."""
    eng = Engine(EngineOpts(windows=8, capacity=CAP))
    inputs = [mc.span_inputs(oracle, prob, i) for i in range(8)]
    for w, (lo, n, st, factors, prior_rec) in enumerate(inputs):
        _load(eng, w, prob, lo, n, st, [(lo, factors)], prior_rec)
    eng.linearize(0)
    cases = [mc.device_case(eng, w, lo, f"spans{mc.SUBSETS[w]}", mc.SUBSETS[w], prior_rec, None, n)
             for w, (lo, n, st, factors, prior_rec) in enumerate(inputs)]
    eng.marginalize()
    for w, case in enumerate(cases):
        got = eng.read_marginal(w)
        # (with the reference sigmas the gauge information is far above the floor: the lift is exactly zero)
        _within(case.name, got, case, oracle.prior_gauge_floor(inputs[w][1]))
        np.testing.assert_array_equal(got["xbar"], case.states[1:4])
    eng.close()


def test_anchor_prior_then_chains(oracle, prob):
    """First marginalisation with the reference prior sigmas at states 0.01 (window 0) and 0.5 rad / 0.5 m (window 1) off the
    prior's mean, then three rounds of marginalize, drop_oldest, set_states(perturbed), linearize(0): the previous marginal
    prior enters with d != 0 (its gradient L d + eta through k2b_priors.inc's marg_delta)."""
    eng = Engine(EngineOpts(windows=2, capacity=CAP))
    placed = {}
    for w, scale in enumerate(mc.CHAIN_SCALES):
        rounds = [mc.chain_inputs(oracle, prob, scale, k) for k in range(4)]
        placed[w] = rounds
        _load(eng, w, prob, mc.CHAIN_LO, mc.CHAIN_N, rounds[0][1], [(lo, f) for lo, _, f in rounds], mc.reference_prior(prob["states"][mc.CHAIN_LO]))
    prev = {}
    for k in range(4):
        if k > 0:
            eng.drop_oldest()
            for w in range(2):
                eng.set_states(w, placed[w][k][0], placed[w][k][1])
        eng.linearize(0)
        cases = []
        for w, scale in enumerate(mc.CHAIN_SCALES):
            lo = placed[w][k][0]
            name = f"anchor-{scale}" if k == 0 else f"chain-{scale}-round{k}"
            prior_rec = mc.reference_prior(prob["states"][lo]) if k == 0 else None
            cases.append(mc.device_case(eng, w, lo, name, mc.CHAIN_SUBSETS[k], prior_rec, prev.get(w), mc.CHAIN_N - k))
        eng.marginalize()
        for w, case in enumerate(cases):
            got = eng.read_marginal(w)
            _within(case.name, got, case, oracle.prior_gauge_floor(mc.CHAIN_N - k))
            np.testing.assert_array_equal(got["xbar"], eng.get_states(w, placed[w][k][0] + 1, 3))     # bit for bit the current states
            prev[w] = dict(L=got["L"], eta=got["eta"], xbar=got["xbar"])
    eng.close()


@pytest.mark.parametrize("outcome", ["accepted", "rejected"])
def test_both_linearisation_buffers(oracle, prob, outcome):
    """The kernel reads the linearisation of buffer sel[w]: after an accepted LM trial that is buffer 1, after a rejected one
    buffer 0 (the rejection is forced by GTSAM's accept rule with an unreachable model fidelity).  Window 1, first slot 63."""
    lo, n = 63, 8
    eng = Engine(EngineOpts(windows=2, capacity=CAP, min_model_fidelity=1e6 if outcome == "rejected" else None))
    st = mc.perturbed(oracle, prob["states"][lo:lo + n], 0.01, 400)
    factors = mc.span_factors(prob, lo, (1, 2, 3), 11)
    prior_rec = mc.reference_prior(prob["states"][lo])
    for w in range(2):
        _load(eng, w, prob, lo, n - w, st[:n - w], [(lo, factors)], prior_rec)
    eng.iterate(1)
    lm = eng.read_lm(1)
    assert (lm["accepted"], lm["rejected"]) == ((1, 0) if outcome == "accepted" else (0, 1)), lm
    moved = np.abs(eng.get_states(1, lo, 4) - st[:4]).max() > 0.0
    assert moved == (outcome == "accepted")
    case = mc.device_case(eng, 1, lo, f"sel-{outcome}", (1, 2, 3), prior_rec, None, n - 1)
    eng.marginalize()
    _within(case.name, eng.read_marginal(1), case, oracle.prior_gauge_floor(n - 1))
    eng.close()


def test_gauge_floor(oracle, prob):
    """Reference sigmas: the floor is not needed yet, an engine with the default floor and one without give the same bits.
    Weak anchor prior (50 m: gauge information 4e-4, below floor_p = 6e-4 of a 6-keyframe window): L = S + lift within the
    extended bound, the four eigenvalues of Q^T L Q at or above the floor, L v = S v off the gauge directions."""
    lo, n, st, factors, weak = mc.weak_inputs(oracle, prob)
    out, case = {}, None
    for floor in (None, 0.0):
        eng = Engine(EngineOpts(windows=2, capacity=CAP, gauge_floor=floor))
        _load(eng, 0, prob, lo, n, st, [(lo, factors)], mc.reference_prior(prob["states"][lo]))
        _load(eng, 1, prob, lo, n, st, [(lo, factors)], weak)
        eng.linearize(0)
        if floor is None:
            case = mc.device_case(eng, 1, lo, "weak-prior-floor", (1, 3), weak, None, n)
        eng.marginalize()
        out[floor] = [eng.read_marginal(w) for w in range(2)]
        eng.close()
    for key in ("L", "eta", "xbar"):
        np.testing.assert_array_equal(out[None][0][key], out[0.0][0][key])
    floor_p = oracle.prior_gauge_floor(n)
    ref, lift, ext = _within("weak-prior-floor", out[None][1], case, floor_p)
    _within("weak-prior-no-floor", out[0.0][1], case)
    assert not np.array_equal(out[None][1]["L"], out[0.0][1]["L"]), "the floor was meant to engage"
    Q = mp_marg.gauge_basis(case.states[1:4], case.gravity)
    ev, slack, lv = mp_marg.floor_properties(out[None][1]["L"], ref, Q, ext, floor_p, np.random.default_rng(5))
    print(f"gauge floor: eigenvalues of Q^T L Q {[float(x) for x in ev]}, floor_p {floor_p:.3e}, admissible shortfall {float(slack):.3e}; "
          f"worst |L v - S v| / bound off the gauge directions {lv:.3e}")
    assert all(x >= floor_p - slack for x in ev) and lv <= 1.0


def test_far_forms_agree_bit_for_bit(oracle, prob):
    """k_marginalize<1> (max_far_factors 8: joint system in LDS) and <2> (far_big_forms with max_far_factors 32: in device
    memory) on a window with two far factors anchored at the leaving keyframe -- one ending at m+2, absorbed like a band
    factor, one at m+5, which becomes a linear row block, comes closer, and folds into m+3 at the third marginalisation."""
    lo, n = 6, 10
    rng = np.random.default_rng(21)
    fa, fb = np.array([lo, lo], dtype=np.int32), np.array([lo + 2, lo + 5], dtype=np.int32)
    far = np.stack([mc.between_record(prob["gt"], int(a), int(b), rng, 1e-4) for a, b in zip(fa, fb)])
    st = mc.perturbed(oracle, prob["states"][lo:lo + n], 0.01, 500)
    outs = []
    for cap, big in ((8, None), (32, 1)):
        eng = Engine(EngineOpts(windows=1, capacity=CAP, max_far_factors=cap, far_big_forms=big))
        _load(eng, 0, prob, lo, n, st, [(lo, mc.span_factors(prob, lo, (1, 3), 12))], mc.reference_prior(prob["states"][lo]))
        eng.set_extra_between(0, fa, fb, far)
        rounds = []
        for k in range(3):
            eng.linearize(0)
            eng.marginalize()
            rounds.append((eng.read_marginal(0), len(eng.get_linear_far(0))))
            eng.drop_oldest()
        rounds.append((None, len(eng.get_linear_far(0))))
        outs.append(rounds)
        eng.close()
    assert [r[1] for r in outs[0]] == [r[1] for r in outs[1]]
    assert outs[0][-1][1] == 0, "the far end has folded into the prior"
    for (a, _), (b, _) in zip(outs[0][:3], outs[1][:3]):
        for key in ("L", "eta", "xbar"):
            np.testing.assert_array_equal(a[key], b[key])


@pytest.mark.parametrize("cap,big", [(8, None), (32, 1)])
def test_far_factor_within_reach_is_absorbed_like_a_band_factor(oracle, prob, cap, big):
    """A far factor anchored at the leaving keyframe that ends at m+2 goes into the 42 x 42 system like a span-2 between factor
    (k_marginalize<1> and <2>, no far end left over): against the reference with that factor linearised by
    mp_lie.between_factor, its rounding counted as input uncertainty."""
    lo, n = 7, 8
    rng = np.random.default_rng(22)
    rec = mc.between_record(prob["gt"], lo, lo + 2, rng, 1e-4)
    st = mc.perturbed(oracle, prob["states"][lo:lo + 4], 0.01, 600)
    prior_rec = mc.reference_prior(prob["states"][lo])
    eng = Engine(EngineOpts(windows=1, capacity=CAP, max_far_factors=cap, far_big_forms=big))
    _load(eng, 0, prob, lo, n, st, [(lo, mc.span_factors(prob, lo, (1, 3), 13))], prior_rec)
    eng.set_extra_between(0, np.array([lo], dtype=np.int32), np.array([lo + 2], dtype=np.int32), rec.reshape(1, -1))
    eng.linearize(0)
    case = mc.device_case(eng, 0, lo, f"far-absorbed-{cap}", (1, 3), prior_rec, None, n, absorbed=[(2, rec)])
    eng.marginalize()
    _within(case.name, eng.read_marginal(0), case, oracle.prior_gauge_floor(n))
    assert len(eng.get_linear_far(0)) == 0
    eng.close()


def test_short_window_is_refused_and_nothing_changes(oracle, prob):
    """A window of 3 keyframes raises; the marginal prior of every window is afterwards what it was, bit for bit."""
    eng = Engine(EngineOpts(windows=2, capacity=CAP))
    for w, n in enumerate((6, 4)):
        lo, _, st, factors, prior_rec = mc.span_inputs(oracle, prob, 7)
        _load(eng, w, prob, lo, n, st, [(lo, factors)], prior_rec)
    eng.linearize(0)
    eng.marginalize()
    eng.drop_oldest()                                     # window 1 is down to 3 keyframes
    eng.linearize(0)
    before = [eng.read_marginal(w) for w in range(2)]
    with pytest.raises(VilFusionError):
        eng.marginalize()
    after = [eng.read_marginal(w) for w in range(2)]
    for a, b in zip(before, after):
        assert a["on"] == b["on"] == 1
        for key in ("L", "eta", "xbar"):
            np.testing.assert_array_equal(a[key], b[key])
    eng.close()
