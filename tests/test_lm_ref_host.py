"""CPU: tests/lm_ref.py, the restated LM decision rule that tests/test_gpu_lm_trace.py holds K5 to.

  1. on every committed case its trace equals vfo_lm's: outcomes and lambda exactly, kept costs within the cost bar;
  2. the case list reaches every outcome, transition, clamp and rule the machine has;
  3. every committed decision is at least MARGIN away from its threshold, MARGIN being >= 1000 x the cost bar, so that a
     correct float64 cost evaluated in another order (the device's) cannot change one;
  4. every mutation of the rule changes the trace of some case (or is recorded as a blind spot);
  5. the cost bar itself: the oracle's float64 cost against 50 digits."""
import math

import numpy as np
import pytest

from tests import lm_ref as lr

_traces = {}


@pytest.fixture(scope="module")
def trace(oracle):
    def get(name, mutation=None):
        key = (name, mutation)
        if key not in _traces:
            _traces[key] = lr.run_host(oracle, lr.BY_NAME[name], mutation=mutation)
        return _traces[key]
    return get


def terminating_trial(tr):
    """the trial at which the window stopped (None: it did not)"""
    return tr.done.index(True) if True in tr.done else None


NAMES = [c.name for c in lr.CASES]


# ---------------------------------------------------------------- 1. against vfo_lm
@pytest.mark.parametrize("name", NAMES)
def test_trace_equals_the_oracles(oracle, trace, name):
    case, tr = lr.BY_NAME[name], trace(name)
    costs, acc, lam, states = lr.run_vfo(oracle, case)
    vfo = "".join("-" if a < 0 else str(a) for a in acc)
    print(f"case {name}: lm_ref {tr.string()}  vfo_lm {vfo}  lambda {tr.final_lam:g} / {lam:g}  cost {tr.cost0:.6e} -> {tr.final_cost:.6e}"
          + ("  (excursion closed at the end)" if tr.closed else ""))
    term = terminating_trial(tr)
    if term is not None:
        # the terminating trial sits at the rounding floor: accept / reject is the last bit's; the number of trials is not
        assert [a >= 0 for a in acc] == [o >= 0 for o in tr.outcomes] and acc[:term] == tr.outcomes[:term]
        upto = term
    else:
        assert acc == tr.outcomes
        assert np.isclose(tr.final_lam, lam, rtol=1e-12, atol=0.0)
        upto = case.K
    kept = tr.cost[:case.K - 1] + [tr.final_cost]         # (vfo_lm's last entry is the cost after an open excursion was undone)
    for t in range(upto):
        assert abs(kept[t] - costs[t + 1]) <= lr.bar(name) * abs(costs[t + 1]), (t, kept[t], costs[t + 1])
    if term is None:
        np.testing.assert_array_equal(tr.final_point[case.lo:case.hi], states)


# ---------------------------------------------------------------- 2. coverage
def test_the_cases_cover_the_machine(trace):
    have = {}

    def mark(what, name):
        have.setdefault(what, []).append(name)

    for name in NAMES:
        case, tr = lr.BY_NAME[name], trace(name)
        o = tr.outcomes
        for v in (0, 1, 2, 3):
            if v in o:
                mark(f"outcome {v}", name)
        if any(a == 0 and b == 1 for a, b in zip(o, o[1:])):
            mark("0 -> 1", name)
        if any(a == 2 and b == 1 for a, b in zip(o, o[1:])):
            mark("excursion ends in 1", name)
        if any(a == 2 and b == 3 for a, b in zip(o, o[1:])):
            mark("excursion ends in 3", name)
        if tr.closed:
            mark("excursion open at the end of the solve", name)
        for t in range(case.K):
            if o[t] in (1, 2) and tr.lam_used[t] == case.lmin and tr.lam[t] == case.lmin:
                mark("lambda held at lmin", name)
            if o[t] in (0, 3) and tr.lam_used[t] == case.lmax and tr.lam[t] == case.lmax:
                mark("lambda held at lmax", name)
        term = terminating_trial(tr)
        if term is not None:
            mark("stopped by the termination rule", name)
            if o[term] == 0:
                mark("... on a rejected trial", name)
        if any(d and out == 0 for d, out in zip(tr.rule_differs, o)):
            mark("fidelity rejects what accept_rel accepts", name)
    wanted = ["outcome 0", "outcome 1", "outcome 2", "outcome 3", "0 -> 1", "excursion ends in 1", "excursion ends in 3",
              "excursion open at the end of the solve", "lambda held at lmin", "lambda held at lmax",
              "stopped by the termination rule", "... on a rejected trial", "fidelity rejects what accept_rel accepts"]
    for w in wanted:
        print(f"{w:45s} {', '.join(sorted(set(have.get(w, [])))) or 'NO CASE'}")
    assert all(w in have for w in wanted)


# ---------------------------------------------------------------- 3. margins
def test_margin_against_the_bar():
    worst = max(lr.bar(n) for n in NAMES)
    print(f"largest cost bar {worst:.2e}, MARGIN {lr.MARGIN:.1e} = {lr.MARGIN / worst:.1e} x")
    assert lr.MARGIN >= 1000.0 * worst


@pytest.mark.parametrize("name", NAMES)
def test_every_decision_clears_the_margin(trace, name):
    case, tr = lr.BY_NAME[name], trace(name)
    term = terminating_trial(tr)
    least = math.inf
    for t in range(case.K):
        if tr.outcomes[t] < 0:
            continue
        m = tr.stop_margin[t] if t == term else min(tr.accept_margin[t], tr.stop_margin[t])
        least = min(least, m)
        assert m >= lr.MARGIN, (t, tr.accept_margin[t], tr.stop_margin[t])
        if tr.rule_differs[t]:      # the accept_rel rule must be as decisive about the trial as the fidelity rule
            ref = tr.cost[t - 1] if t else tr.cost0
            assert abs(tr.trial_cost[t] - ref * (1.0 + case.accept_rel)) / ref >= lr.MARGIN
    print(f"case {name} ({tr.string()}): least margin {least:.3g}")


# ---------------------------------------------------------------- 4. mutations
def test_every_mutation_is_caught(oracle, trace):
    blind = []
    for mut in lr.MUTATIONS:
        caught = [n for n in NAMES if trace(n, mut).key() != trace(n).key()]
        detail = ", ".join(f"{n} ({trace(n, mut).string()})" for n in caught)
        print(f"{mut:32s} {detail or 'no committed case'}")
        if not caught:
            blind.append(mut)
    assert tuple(blind) == lr.BLIND_SPOTS
    # ... and the blind spot by the scripted sequence, in the machine alone
    name, fail_at = lr.SCRIPTED_FAIL
    base = lr.run_host(oracle, lr.BY_NAME[name], fail_at=fail_at)
    mutd = lr.run_host(oracle, lr.BY_NAME[name], mutation="failed_solve_keeps_excursion", fail_at=fail_at)
    print(f"failed_solve_keeps_excursion, scripted on {name} (solve of trial {fail_at[0]} declared failed): {base.string()} against {mutd.string()}")
    assert base.outcomes[fail_at[0]] == 3 and mutd.outcomes[fail_at[0]] == 0 and base.counters[3] == 1


# ---------------------------------------------------------------- 5. the bar
@pytest.mark.parametrize("name", NAMES)
def test_cost_bar(oracle, trace, name):
    """S: the oracle's float64 cost against 50 digits at the first three trial points"""
    from tests import mp_lie as ml
    case, tr = lr.BY_NAME[name], trace(name)
    prob = lr.problem(oracle, case)
    S = 0.0
    for states, c in tr.trial_points:
        exact = lr.mp_cost(prob, states, case.lo, case.hi)
        S = max(S, float(abs(ml.mp.mpf(c) - exact) / exact))
        assert lr.window_at(oracle, prob, states, case.lo, case.hi).cost() == c      # (vfo_cost and vfo_assemble: one sum)
    print(f"case {name}: S = {S:.2e} over {len(tr.trial_points)} trial points (committed {lr.S_CASE[name]:.1e}); bar {lr.bar(name):.2e}")
    assert len(tr.trial_points) == 3 or name == "stop_rej"
    assert S <= lr.S_CASE[name] <= max(4.0 * S, 4.0 * lr.EPS)


# ---------------------------------------------------------------- the solve's ends
def test_begin_and_end_of_a_solve():
    exc, plain = lr.Machine(lr.BY_NAME["exc_ok"]), lr.Machine(lr.BY_NAME["rej_acc"])
    for m in (exc, plain):
        m.begin_solve(100.0, "a")
        assert m.lam == m.p.lam0
        assert m.step(50.0, True, point="b") == 1
        assert not m.end_solve()
        lam = m.lam
        m.begin_solve(50.0, "b")
        assert m.lam == (lam if m.p.W > 0 else m.p.lam0)      # an engine that runs excursions carries its damping; others do not
    exc.begin_solve(50.0, "b")
    assert exc.step(80.0, True, point="c") == 2 and exc.point == "c" and exc.prov == 1
    assert exc.end_solve() and exc.point == "b" and exc.cost == 50.0 and exc.prov == 0


def test_two_solves_of_an_excursion_engine_are_one(oracle, trace):
    """with the damping carried, iterate(3) then iterate(1) is iterate(4) where no excursion is open at the cut; cut inside an
    excursion, the second solve starts from the point the excursion left with the damping it had reached"""
    import dataclasses
    case = lr.BY_NAME["exc_ok"]
    whole = lr.run_host(oracle, dataclasses.replace(case, K=4))
    split = lr.run_host(oracle, case, solves=(3, 1))
    assert split.key() == whole.key() and split.final_cost == whole.final_cost
    cut = lr.run_host(oracle, case, solves=(1, 1))
    print(f"exc_ok as iterate(1), iterate(1): {cut.string()}, lambda used {cut.lam_used}")
    assert cut.outcomes[0] == 2 and cut.lam_used[1] == cut.lam[0] != case.lam0
    plain = lr.run_host(oracle, lr.BY_NAME["rej_acc"], solves=(2, 1))
    assert plain.lam_used == [case.lam0 * 0 + 1.0, 10.0, 1.0]          # lm_excursion = 0: every solve starts from lambda0
