"""-m gpu: K5's decision kernels (k_decide, k_model_change, k_close_excursion, k_reset_lambda) trial by trial at windows of
33 to 40 keyframes, against tests/lm_ref.py: the rule restated as a plain state machine, its cases chosen and their margins
measured on the CPU (tests/test_lm_ref_host.py).

The reference of a trial is built from what the DEVICE holds: its current states and its increment give the trial point
(oracle.retract) and the trial's cost (the oracle's Window), so neither the accuracy of the band solve nor the drift of a
chaotic start is part of the comparison.  Every decision must then be at least lm_ref.MARGIN away from its threshold (a
failure, never a skip), and outcome, damping, kept cost, provisional count and the BITS of the kept states must be the
machine's.

  a. staged: reset_lambda, linearize(0), decide(init), then { assemble, solve, retract, linearize(1), decide } x K,
     close_excursions; afterwards the same as one iterate(K) on a fresh engine, bit for bit
  b. the same on the window [3, 36) of 40 loaded keyframes: the 7 keyframes outside keep their bits in both buffers
  c. iterate(k) for k = 0 .. K, each on a fresh engine (k_model_change, k_reset_lambda and the close at the end of a solve
     have no stage call; engines without excursions replay a captured graph); the damping carried between two solves
  d. batches of 3 and of 66 windows (the 256-thread form of k_decide and k_close_excursion), one of them a window whose
     solve fails: bit for bit the single-window traces
  e. the termination rule beside a window that keeps taking trials

No branch is scripted through set_states.  Reached by no test here: a solve that fails while an excursion is open
(lm_ref.BLIND_SPOTS).  refine_iterations = 0 and lm_excursion explicit on every engine."""
import math

import numpy as np
import pytest

from tests import helpers
from tests import lm_ref as lr
from vil_sensor_fusion_amd import synth

pytestmark = pytest.mark.gpu
CAP = 48
RETRACT_TOL = 1e-12          # x max(1, |state|): the bar of test_gpu_lie_edges.py::test_retract_of_large_increments
_share = {}                  # largest share of the cost bar seen, by case


def make_engine(case, windows=1, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    opts = dict(lambda0=case.lam0, lambda_up=case.up, lambda_down=case.down, lambda_min=case.lmin, lambda_max=case.lmax,
                lm_excursion=case.W, refine_iterations=0, accept_rel=case.accept_rel, min_model_fidelity=case.min_fidelity)
    opts.update(kw)
    eng = Engine(EngineOpts(windows=windows, capacity=CAP, **opts))
    if case.rel_tol > 0.0 or case.abs_tol > 0.0:
        eng.set_convergence(case.rel_tol, case.abs_tol)
    return eng


def load(oracle, eng, w, case):
    helpers.load_engine(eng, w, lr.problem(oracle, case), lo=case.lo, hi=case.hi)


BAD_N = 16


def load_bad(oracle, eng, w):
    """a window whose every solve fails: neither prior nor between factors, and (as test_indeterminate_system_is_flagged
    makes its failure) a NaN in one state.  The NaN is needed: without prior and between factors alone the damped system is
    positive definite from lambda = 1e-5 on (oracle.band_solve returns 0), only the undamped one is not."""
    prob = helpers.build_problem(oracle, synth.make_sequence(50, BAD_N))
    st = prob["states"].copy()
    st[5, 4] = np.nan
    eng.set_states(w, 0, st)
    eng.set_imu(w, 1, prob["imu"][1:])
    eng.set_range(w, 0, BAD_N)


def read_window(eng, w, n):
    return dict(lm=eng.read_lm(w), exc=eng.read_excursions(w), states=eng.get_states(w, 0, n), est=eng.get_estimate(w, 0, n))


def counters(r):
    return (r["lm"]["accepted"], r["lm"]["rejected"], r["exc"][0], r["lm"]["solve_failures"])


def staged(eng, wins, K):
    """the stage calls in the order of vf_engine_iterate.  wins: {window: (lo, hi, keyframes loaded)}.
    Returns (after decide(init), [per trial {window: (before decide, after decide)}], after close_excursions)"""
    eng.reset_lambda()
    eng.linearize(0)
    eng.decide(True)
    init = {w: read_window(eng, w, n) for w, (lo, hi, n) in wins.items()}
    recs = []
    for _ in range(K):
        eng.assemble()
        eng.solve()
        eng.retract()
        eng.linearize(1)
        pre = {w: dict(read_window(eng, w, n), delta=eng.read_delta(w, lo, hi - lo)) for w, (lo, hi, n) in wins.items()}
        eng.decide(False)
        recs.append({w: (pre[w], read_window(eng, w, n)) for w, (lo, hi, n) in wins.items()})
    if eng.opts.lm_excursion > 0:
        eng.close_excursions()
    return init, recs, {w: read_window(eng, w, n) for w, (lo, hi, n) in wins.items()}


def outcome_of(pre, post):
    """the outcome of a trial from the counters: exactly one of accepted / rejected / provisional moved; a rejection that
    emptied an open excursion is 3"""
    d = np.subtract(counters(post), counters(pre))
    assert d[0] + d[1] + d[2] == 1 and min(d) >= 0 and d[3] in (0, 1), d
    if d[0]:
        return 1
    if d[2]:
        return 2
    return 3 if pre["exc"][1] > 0 and post["exc"][1] == 0 else 0


def retract_error(oracle, states, delta, got):
    """(oracle.retract(states, delta), largest |got - that| / max(1, |that|) per keyframe, q and -q being one rotation)"""
    ref = lr.retract_all(oracle, states, delta)
    worst = 0.0
    for r, g in zip(ref, got):
        a = r.copy()
        if np.dot(a[:4], g[:4]) < 0:
            a[:4] = -a[:4]
        worst = max(worst, np.abs(g - a).max() / max(1.0, np.abs(a).max()))
    return ref, worst


def note_share(name, got, ref):
    share = abs(got - ref) / (lr.bar(name) * abs(ref))
    _share[name] = max(_share.get(name, 0.0), share)
    return share


def check_staged(oracle, case, init, recs, closed, w=0):
    """a, b: every trial of a staged run against the machine (closed = None: the trials only)"""
    prob = lr.problem(oracle, case)
    lo, hi, n = case.lo, case.hi, case.n
    loaded = prob["states"]
    outside = [k for k in range(n) if k < lo or k >= hi]
    np.testing.assert_array_equal(init[w]["states"], loaded)
    np.testing.assert_array_equal(init[w]["est"], loaded)
    m = lr.Machine(case)
    c0 = lr.window_at(oracle, prob, loaded, lo, hi).cost()
    assert note_share(case.name, init[w]["lm"]["cost"], c0) <= 1.0
    assert init[w]["lm"]["lam"] == case.lam0 and counters(init[w]) == (0, 0, 0, 0) and init[w]["exc"][1] == 0
    m.begin_solve(c0, init[w]["states"])
    trace, dev_ref, least = "", None, math.inf
    for t, rec in enumerate(recs):
        pre, post = rec[w]
        assert np.isclose(pre["lm"]["lam"], m.lam, rtol=1e-12, atol=0.0), (t, pre["lm"]["lam"], m.lam)     # the damping the trial ran with
        np.testing.assert_array_equal(pre["states"], m.point)
        ref, e = retract_error(oracle, pre["states"][lo:hi], pre["delta"], pre["est"][lo:hi])
        assert e <= RETRACT_TOL, (t, e)
        trial = pre["states"].copy()
        trial[lo:hi] = ref
        c_ref = lr.window_at(oracle, prob, trial, lo, hi).cost()
        solved = post["lm"]["solve_failures"] == pre["lm"]["solve_failures"]
        mg = lr.margin(c_ref, m, solved)
        least = min(least, mg)
        assert mg >= lr.MARGIN, (t, mg)
        opening = m.prov == 0
        out = m.step(c_ref, solved, point=pre["est"])
        if out == 2 and opening:
            dev_ref = pre["lm"]["cost"]
        trace += str(out)
        assert outcome_of(pre, post) == out, (t, trace, counters(pre), counters(post))
        assert np.isclose(post["lm"]["lam"], m.lam, rtol=1e-12, atol=0.0), (t, post["lm"]["lam"], m.lam)
        assert note_share(case.name, post["lm"]["cost"], m.cost) <= 1.0, (t, post["lm"]["cost"], m.cost)
        assert post["exc"][1] == m.prov and counters(post) == m.counters()
        # 0: the bits from before the trial; 1, 2: the bits of the trial buffer; 3: the bits the excursion left, all 16 words
        np.testing.assert_array_equal(post["states"], m.point)
        if out == 0:
            assert post["lm"]["cost"] == pre["lm"]["cost"]
        if out == 3:
            assert post["lm"]["cost"] == dev_ref
        for r in (pre, post):
            np.testing.assert_array_equal(r["states"][outside], loaded[outside])
            np.testing.assert_array_equal(r["est"][outside], loaded[outside])
    last = recs[-1][w][1]
    if case.W > 0 and closed is not None:
        restored = m.end_solve()
        np.testing.assert_array_equal(closed[w]["states"], m.point)
        np.testing.assert_array_equal(closed[w]["states"][outside], loaded[outside])
        np.testing.assert_array_equal(closed[w]["est"][outside], loaded[outside])
        assert closed[w]["exc"][1] == 0 and counters(closed[w]) == counters(last) and closed[w]["lm"]["lam"] == last["lm"]["lam"]
        assert closed[w]["lm"]["cost"] == (dev_ref if restored else last["lm"]["cost"])
        trace += " closed" if restored else ""
    print(f"case {case.name}: {trace}; least margin {least:.3g}; largest share of the cost bar {_share[case.name]:.3f}")
    return trace


STAGED = ["rej_acc", "rej_acc8", "exc_ok", "exc_ok3", "exc_fail", "all_rej", "rel_half", "range"]


# ---------------------------------------------------------------- a, b
@pytest.mark.parametrize("name", STAGED)
def test_staged_trace(oracle, name):
    case = lr.BY_NAME[name]
    eng = make_engine(case)
    load(oracle, eng, 0, case)
    init, recs, closed = staged(eng, {0: (case.lo, case.hi, case.n)}, case.K)
    eng.close()
    trace = check_staged(oracle, case, init, recs, closed)
    assert trace.split()[0] == lr.run_host(oracle, case).string()          # (the trace the case was committed for)
    if name == "range":
        assert "2" in trace and "3" in trace and trace.endswith("closed")
    # ... and one iterate(K) on a fresh engine: the same bits
    eng = make_engine(case)
    load(oracle, eng, 0, case)
    eng.iterate(case.K)
    whole = read_window(eng, 0, case.n)
    eng.close()
    np.testing.assert_array_equal(whole["states"], closed[0]["states"])
    assert whole["lm"] == closed[0]["lm"] and whole["exc"] == closed[0]["exc"]


# ---------------------------------------------------------------- c
_prefix = {}


def prefixes(oracle, case):
    """iterate(k), k = 0 .. K, each on a fresh engine; engines without excursions replay a captured graph"""
    if case.name not in _prefix:
        out = []
        for k in range(case.K + 1):
            eng = make_engine(case, use_hip_graph=case.W == 0)
            load(oracle, eng, 0, case)
            eng.iterate(k)
            r = read_window(eng, 0, case.n)
            r["delta"] = eng.read_delta(0, case.lo, case.hi - case.lo)
            r["graph"] = eng.graph_info()
            eng.close()
            out.append(r)
        _prefix[case.name] = out
    return _prefix[case.name]


def symbol(prev, cur):
    d = np.subtract(counters(cur), counters(prev))
    assert d[0] + d[1] + d[2] <= 1 and min(d) >= 0, d
    return "1" if d[0] else "2" if d[2] else "R" if d[1] else "-"


SYMBOL = {0: "R", 3: "R", 1: "1", 2: "2", -1: "-"}


@pytest.mark.parametrize("name", [c.name for c in lr.CASES])
def test_prefix_runs(oracle, name):
    case = lr.BY_NAME[name]
    prob = lr.problem(oracle, case)
    lo, hi = case.lo, case.hi
    host = lr.run_host(oracle, case)
    pre = prefixes(oracle, case)
    term = host.done.index(True) if True in host.done else None
    np.testing.assert_array_equal(pre[0]["states"], prob["states"])
    assert pre[0]["lm"]["lam"] == case.lam0
    got = "".join(symbol(pre[k - 1], pre[k]) for k in range(1, case.K + 1))
    print(f"case {name}: device {got}, lm_ref {host.string()}" + (f", stopped at trial {term}" if term is not None else ""))
    for k in range(1, case.K + 1):
        t = k - 1
        assert pre[k]["exc"][1] == 0                                   # (the end of the solve leaves no excursion open)
        if case.W == 0:
            assert pre[k]["graph"][0] and pre[k]["graph"][2] >= 1      # (the replayed graph)
        if term is not None and t == term:
            assert got[t] in "1R"                                      # (accept / reject at the floor: the last bit's)
            continue
        if term is not None and t > term:
            # further trials of the same call change no counter and no state
            assert got[t] == "-" and pre[k]["lm"] == pre[k - 1]["lm"]
            np.testing.assert_array_equal(pre[k]["states"], pre[k - 1]["states"])
            continue
        assert got[t] == SYMBOL[host.outcomes[t]], (t, got, host.string())
        assert np.isclose(pre[k]["lm"]["lam"], host.lam[t], rtol=1e-12, atol=0.0), (t, pre[k]["lm"]["lam"], host.lam[t])
        if case.W > 0:
            before = host.prov[t - 1] if t else 0
            if host.prov[t] > 0:        # the prefix ends inside an excursion: the point it left, from the prefix that ended there
                j = k - host.prov[t]
            elif host.outcomes[t] == 3:
                j = t - before
            else:
                continue
            np.testing.assert_array_equal(pre[k]["states"], pre[j]["states"])
            assert pre[k]["lm"]["cost"] == pre[j]["lm"]["cost"]
    if case.W > 0:
        return
    # engines without excursions: prefix k - 1 holds the states trial k started from and read_delta its increment, so every
    # trial has a reference built from the device's own data, the fidelity rule's prediction included
    m = lr.Machine(case)
    c0 = lr.window_at(oracle, prob, pre[0]["states"], lo, hi).cost()
    assert note_share(name, pre[0]["lm"]["cost"], c0) <= 1.0
    m.begin_solve(c0, pre[0]["states"])
    least = math.inf
    for k in range(1, case.K + 1):
        if m.done:
            break
        cur, d = pre[k - 1]["states"], pre[k]["delta"]
        trial = cur.copy()
        trial[lo:hi] = lr.retract_all(oracle, cur[lo:hi], d)
        c = lr.window_at(oracle, prob, trial, lo, hi).cost()
        predicted = lr.predicted_decrease(oracle, prob, cur, lo, hi, d) if case.min_fidelity > 0.0 else None
        solved = pre[k]["lm"]["solve_failures"] == pre[k - 1]["lm"]["solve_failures"]
        stopping = (case.rel_tol > 0.0 or case.abs_tol > 0.0) and solved and m.stops(c)
        mg = lr.stop_margin(m, c, solved) if stopping else lr.margin(c, m, solved, predicted)
        least = min(least, mg)
        assert mg >= lr.MARGIN, (k, mg)
        out = m.step(c, solved, predicted, point=trial)
        assert m.done == stopping
        if stopping:
            assert got[k - 1] in "1R"
            continue
        assert got[k - 1] == SYMBOL[out], (k, got, out)
        assert np.isclose(pre[k]["lm"]["lam"], m.lam, rtol=1e-12, atol=0.0)
        assert note_share(name, pre[k]["lm"]["cost"], m.cost) <= 1.0, (k, pre[k]["lm"]["cost"], m.cost)
        if out == 0:
            np.testing.assert_array_equal(pre[k]["states"], cur)
            assert pre[k]["lm"]["cost"] == pre[k - 1]["lm"]["cost"]
        else:
            _, e = retract_error(oracle, cur[lo:hi], d, pre[k]["states"][lo:hi])
            assert e <= RETRACT_TOL, (k, e)
    assert m.counters() == counters(pre[case.K]) or term is not None
    print(f"case {name}: least margin from the device's own trial points {least:.3g}; largest share of the cost bar {_share[name]:.3f}")


def test_damping_carries_between_solves(oracle):
    """What the engine does, established here: with lm_excursion > 0 EVERY window's damping goes on from one vf_engine_iterate
    to the next (vf_engine_close_excursions marks them all), whether or not the solve ended inside an excursion; with
    lm_excursion = 0 every solve starts from lambda0.  lm_ref.Machine.end_solve() is pinned to that."""
    case = lr.BY_NAME["exc_ok"]
    # cut where no excursion is open (221 | 1): two solves are one
    eng = make_engine(case)
    load(oracle, eng, 0, case)
    eng.iterate(3)
    mid = read_window(eng, 0, case.n)
    eng.iterate(1)
    two = read_window(eng, 0, case.n)
    eng.close()
    whole = prefixes(oracle, case)
    host = lr.run_host(oracle, case, solves=(3, 1))
    print(f"exc_ok, iterate(3) then iterate(1): lambda {mid['lm']['lam']:g} -> {two['lm']['lam']:g}; one iterate(4): {whole[4]['lm']['lam']:g}; "
          f"from lambda0 the fourth trial would have run with {case.lam0:g}")
    assert mid["lm"] == whole[3]["lm"]
    assert np.isclose(two["lm"]["lam"], host.lam[3], rtol=1e-12, atol=0.0) and counters(two) == host.counters
    assert two["lm"] == whole[4]["lm"] and two["exc"] == whole[4]["exc"]
    np.testing.assert_array_equal(two["states"], whole[4]["states"])
    # cut inside an excursion (2 | 2): the second solve starts from the point the excursion left, with the damping it reached
    eng = make_engine(case)
    load(oracle, eng, 0, case)
    eng.iterate(1)
    eng.iterate(1)
    cut = read_window(eng, 0, case.n)
    eng.close()
    host = lr.run_host(oracle, case, solves=(1, 1))
    assert host.string() == "22" and host.lam_used[1] == host.lam[0]
    assert np.isclose(cut["lm"]["lam"], host.lam[1], rtol=1e-12, atol=0.0) and counters(cut) == host.counters
    np.testing.assert_array_equal(cut["states"], lr.problem(oracle, case)["states"])
    # no excursions: from lambda0 again
    case = lr.BY_NAME["rej_acc"]
    eng = make_engine(case)
    load(oracle, eng, 0, case)
    eng.iterate(2)
    eng.iterate(1)
    lam = eng.read_lm(0)["lam"]
    eng.close()
    host = lr.run_host(oracle, case, solves=(2, 1))
    assert host.lam_used[2] == case.lam0 and np.isclose(lam, host.lam[2], rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------- d
def strip(recs, w):
    """what a window's trace is compared by, bit for bit: per trial the damping, cost, counters, open excursion and states
    before and after the decision, the trial buffer and the increment"""
    return [[(r["lm"], r["exc"], r["states"].tobytes(), r["est"].tobytes()) for r in rec[w]] + [rec[w][0]["delta"].tobytes()] for rec in recs]


@pytest.mark.parametrize("names,K", [(("rej_acc", "rej_acc8"), 12), (("exc_ok", "exc_fail"), 6)])
def test_batches_bit_for_bit(oracle, names, K):
    cases = [lr.BY_NAME[n] for n in names]
    base = cases[0]
    assert all((c.lam0, c.up, c.down, c.lmin, c.lmax, c.W, c.accept_rel) == (base.lam0, base.up, base.down, base.lmin, base.lmax, base.W, base.accept_rel) for c in cases)
    # (chunks = 1 on every engine: whole-window sweeps, the one solve form all three batch sizes share -- the increments are
    # then the same bits, and what is left to differ is K5's own reduction and indexing)
    singles = []
    for c in cases:
        eng = make_engine(base, chunks=1)
        load(oracle, eng, 0, c)
        init, recs, closed = staged(eng, {0: (c.lo, c.hi, c.n)}, K)
        eng.close()
        check_staged(oracle, c, init, recs[:c.K], None)          # (the sweeps' increments; test_staged_trace has the default form's)
        singles.append((init[0], strip(recs, 0), closed[0]))
    for B, where in ((3, (0, 1, 2)), (66, (0, 1, 65))):
        eng = make_engine(base, windows=B, chunks=1)
        wins = {}
        for w, c in zip(where, cases):
            load(oracle, eng, w, c)
            wins[w] = (c.lo, c.hi, c.n)
        load_bad(oracle, eng, where[2])
        wins[where[2]] = (0, BAD_N, BAD_N)
        init, recs, closed = staged(eng, wins, K)
        eng.close()
        for i, w in enumerate(where[:2]):
            assert init[w]["lm"] == singles[i][0]["lm"]
            assert strip(recs, w) == singles[i][1], f"window {w} of {B}"
            assert closed[w]["lm"] == singles[i][2]["lm"]
            np.testing.assert_array_equal(closed[w]["states"], singles[i][2]["states"])
        # the window whose solves fail: no excursion is open, so 0 at every trial whatever W; lambda climbs to the clamp
        m = lr.Machine(base)
        m.begin_solve(math.nan)
        bad = where[2]
        for t, rec in enumerate(recs):
            pre, post = rec[bad]
            assert m.step(math.nan, False) == 0 and outcome_of(pre, post) == 0
            assert np.isclose(post["lm"]["lam"], m.lam, rtol=1e-12, atol=0.0) and counters(post) == m.counters() == (0, t + 1, 0, t + 1)
            assert post["exc"][1] == 0
            np.testing.assert_array_equal(post["states"], init[bad]["states"])
        assert m.lam == base.lmax and recs[-2][bad][1]["lm"]["lam"] == base.lmax
        print(f"{B} windows, {names}: windows {where[:2]} bit for bit their single-window traces; window {bad}: {K} failed solves, lambda {m.lam:g}")


# ---------------------------------------------------------------- e
def test_termination_beside_a_window_that_goes_on(oracle):
    stop, rej = lr.BY_NAME["stop"], lr.BY_NAME["all_rej"]
    assert (stop.lam0, stop.lmax, stop.W, stop.K) == (rej.lam0, rej.lmax, rej.W, rej.K)
    host = lr.run_host(oracle, stop)
    ran = sum(o >= 0 for o in host.outcomes)
    eng = make_engine(stop, windows=2)
    load(oracle, eng, 0, stop)
    load(oracle, eng, 1, rej)
    eng.iterate(stop.K)
    a, b = read_window(eng, 0, stop.n), read_window(eng, 1, rej.n)
    eng.close()
    print(f"stop: {a['lm']['accepted']} accepted + {a['lm']['rejected']} rejected of {stop.K} trials (lm_ref: {ran}); beside it {b['lm']['rejected']} rejected")
    assert a["lm"]["accepted"] + a["lm"]["rejected"] == ran < stop.K
    assert b["lm"]["accepted"] == 0 and b["lm"]["rejected"] == stop.K and b["lm"]["lam"] == rej.lmax
    np.testing.assert_array_equal(b["states"], lr.problem(oracle, rej)["states"])
    # the trials after the window stopped changed nothing: the bits of iterate(ran) alone (whose own margins
    # test_prefix_runs[stop] holds to MARGIN)
    alone = prefixes(oracle, stop)[ran]
    assert a["lm"] == alone["lm"]
    np.testing.assert_array_equal(a["states"], alone["states"])
