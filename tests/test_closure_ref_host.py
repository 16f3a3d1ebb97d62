"""What fixes the numbers of tests/closure_ref.py, on the CPU (no GPU): the candidate lists are what they are for, the floor
S_JOINT of three correct float64 evaluations of Sigma_J is the written table, the float64 restatement of nis stays within the
written NIS_FLOOR of mpmath, and the bars 16 x S_JOINT and 16 x NIS_FLOOR would catch a Sigma_J without its downdate, with its cross
block transposed or zeroed, without the marginal prior, and Jacobians swapped -- or closure_ref.BLIND says where they would not.
tests/test_gpu_closure_gate.py holds the device to the same tables."""
import numpy as np
import pytest

from tests import closure_ref as cl
from tests import cov_ref as cr

_refs = {}


@pytest.fixture(scope="module")
def ref(oracle):
    """(cov_ref.reference, closure_ref.reference) of a case, built once"""
    def get(name):
        if name not in _refs:
            f = cr.reference(oracle, cr.make_case(oracle, name))
            _refs[name] = (f,) + cl.reference(oracle, f)
        return _refs[name]
    return get


def test_candidates_reach_what_they_are_for(ref):
    assert set(cl.S_JOINT) == set(cr.CASES)
    for name in cr.CASES:
        case = ref(name)[0]["case"]
        c = cl.candidates(case)
        assert len(c) <= 4 and len(set(c)) == len(c)
        assert all(case.lo <= a <= b < case.hi for a, b in c)
        if case.n >= 2:
            assert {(case.lo, case.hi - 1), (case.lo, case.lo + 1), (case.hi - 2, case.hi - 1)} <= set(c)
            assert any(b == a + 1 for a, b in c)                                      # an adjacent candidate on every case
        if case.n >= 6:
            assert len(c) == 4                                                           # the cap
            assert (case.lo + 1, case.hi - 2) in c or case.far is not None
    assert cl.candidates(ref("L1")[0]["case"]) == [(0, 0)] and cl.testable(ref("L1")[0]["case"]) == []
    m = ref("M12")[0]["case"]
    assert m.marg is not None and any(a == m.lo for a, _ in cl.candidates(m))           # the marginal prior's keyframe
    for name in cr.FAR_CASES:
        case = ref(name)[0]["case"]
        assert cl.FAR_PAIR in cl.candidates(case) and cl.FAR_PAIR in set(zip(case.far[0].tolist(), case.far[1].tolist()))


@pytest.mark.parametrize("name", cr.CASES)
def test_floor_is_the_written_constant(ref, name):
    f, cref, s = ref(name)
    if cl.S_JOINT[name] is None:
        assert s is None and not cref
        return
    for (a, b), c in cref.items():
        print(f"case {name}, candidate ({a}, {b}): " + ", ".join(f"{k} {v:.3e}" for k, v in c["errs"].items()))
    print(f"case {name}: S_JOINT measured {s:.3e} (written {cl.S_JOINT[name]:.2e}, bar {cl.bar(name):.2e}; cov_ref.S {cr.S[name]:.2e})")
    assert s <= cl.S_JOINT[name] <= 1.25 * s
    assert f["last"] <= cl.S_JOINT[name] / 100.0                        # the reference has converged below the floor


def test_nis_floor_is_the_written_constant(ref):
    """nis_f64 fed the reference Sigma_J against mpmath fed the same: the worst relative error is NIS_FLOOR; xi within XI_BAR and
    nis_measurement within measurement_bar on every case -- the bars the device is held to are ones a float64 evaluation meets"""
    worst, where = 0.0, None
    for name in cr.CASES:
        case = ref(name)[0]["case"]
        for (a, b), c in ref(name)[1].items():
            for k in cl.KINDS:
                m, d = c["mp"][k], c["f64"][k]
                e = abs(d["nis"] - m["nis"]) / m["nis"]
                ex = float(np.max(np.abs(d["xi"] - m["xi"])))
                em = abs(d["nis_measurement"] - m["nis_measurement"])
                print(f"case {name} ({a}, {b}) {k:10s}: nis {m['nis']:.6e} rel. error {e:.2e}; xi {ex:.1e}; nis_measurement {em:.1e} "
                      f"(bar {cl.measurement_bar(c['recs'][k], m['nis_measurement']):.1e})")
                assert ex <= cl.XI_BAR and em <= cl.measurement_bar(c["recs"][k], m["nis_measurement"])
                assert (m["nis"] > 16.81) == (k == "gross") and m["nis"] <= m["nis_measurement"]
                if e > worst:
                    worst, where = e, (name, (a, b), k)
    print(f"worst relative nis error of the float64 restatement {worst:.3e} at {where}; NIS_FLOOR {cl.NIS_FLOOR:.1e}; NIS_BAR {cl.NIS_BAR:.2e}")
    assert worst <= cl.NIS_FLOOR <= 1.25 * worst


@pytest.mark.parametrize("name", [c for c in cr.CASES if cl.S_JOINT[c] is not None])
def test_the_bars_can_fail(oracle, ref, name):
    """every mutation of closure_ref.mutations lands beyond 10 x its bar but for closure_ref.BLIND, whose entries are held to what
    they record.  The downdate left out: G17 must see it.  Sigma_ab zeroed: every adjacent candidate must see it.  The marginal
    prior left out: M12."""
    f, cref, _ = ref(name)
    case = f["case"]
    muts = cl.mutations(oracle, f, cref)
    kinds = {what for what, _, _ in muts}
    want = {"Sigma_ab transposed", "Sigma_ab zeroed", "Ja and Jb swapped, consistent", "Ja and Jb swapped, gross"}
    want |= {"the downdate left out"} if case.far is not None else set()
    want |= {"the marginal prior left out"} if case.marg is not None else set()
    assert kinds == want and (name != "M12" or "the marginal prior left out" in kinds) and (name != "G17" or "the downdate left out" in kinds)
    for what, (a, b), m in muts:
        key = (name, what, (a, b))
        print(f"case {name}, ({a}, {b}), {what}: {m:.3g} x the bar" + (" (BLIND)" if key in cl.BLIND else ""))
        if key in cl.BLIND:
            assert m <= cl.BLIND[key] <= 1.25 * m and cl.BLIND[key] <= 10.0
            assert not (name == "G17" and what == "the downdate left out")
            assert not (what == "Sigma_ab zeroed" and b == a + 1)
            assert not (name == "M12" and what == "the marginal prior left out" and a == case.lo)
        else:
            assert m > 10.0, key
    assert {k[0] for k in cl.BLIND} <= set(cr.CASES)
