"""What fixes the numbers of tests/direct_ref.py, on the CPU (no GPU): the extended-precision reference has converged on every
case, the floor S of three correct float64 evaluations of the normal equations is the written table, the elimination order is
no term of its own, and the bar 16 x S would catch normal equations that are wrong in one row class.
tests/test_gpu_direct_small.py holds every form of the direct band solve to the same table."""
import numpy as np
import pytest

from tests import direct_ref as dr
from tests import refine_ref as rr

_cases, _refs = {}, {}
IDS = [f"{c}-{lam:g}" for c, lam in dr.KEYS]


@pytest.fixture(scope="module")
def ref(oracle):
    def get(name, lam):
        if name not in _cases:
            _cases[name] = dr.make_case(oracle, name)
        if (name, lam) not in _refs:
            _refs[(name, lam)] = dr.reference(oracle, _cases[name], lam)
        return _refs[(name, lam)]
    return get


def test_ladder_has_the_chunk_edges():
    """the lengths at which vf_chunk_geometry goes to 2, 3 and 4 chunks, for chunks = 4 and for the fitted count (chunks = 0: at
    most 96 on engines of up to 128 windows), with the length below each"""
    from vil_sensor_fusion_amd.distributed import chunk_geometry
    for chunks, fit in ((4, False), (96, True)):
        count = {n: len(chunk_geometry(n, chunks, fit)) for n in range(2, 129)}
        for c, edge in dr.CHUNK_EDGES.items():
            assert min(n for n, k in count.items() if k == c) == edge and count[edge - 1] == c - 1
            assert edge in dr.LADDER and edge - 1 in dr.LADDER
    assert set(dr.LADDER) >= {2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 33}


def test_cases_reach_what_they_are_for(ref):
    for name, (lo, hi) in dr.OFFSETS.items():
        c = ref(name, rr.LAMBDA)["case"]
        assert (c.lo, c.hi) == (lo, hi) and lo % 64 != 0 and (lo % 8 != 0 or name == "O8")      # (O8: on the tile, off the 64-slot block)
        assert np.any(c.prob["btw_a"] < lo) and np.any(c.prob["btw_b"] >= hi) and c.prior_k == lo
    b = ref("B", rr.LAMBDA)["case"]
    assert (b.lo, b.hi) == (3, 131)
    far = ref("F17", rr.LAMBDA)["rows"].find("far")
    assert len(far) == 3 and far[0][1] == far[1][1] and far[2][2] == 16             # two slots on one keyframe, one ends at the last
    for name in dr.MARG_CASES:
        m = ref(name, rr.LAMBDA)["case"]
        assert m.prior_k is None and np.abs(m.marg["L"][21:27]).max() > 0.0         # the prior's rows of keyframe lo + 2 are alive
    assert ref("M12", rr.LAMBDA)["case"].n == 12 and ref("L2", rr.LAMBDA)["rows"].find("btw") == []


@pytest.mark.parametrize("key", dr.KEYS, ids=IDS)
def test_reference_converged(ref, key):
    f = ref(*key)
    print(f"case {key[0]}, lambda {key[1]:g}: {f['rows'].J.shape[0]} rows, {f['rows'].J.shape[1]} columns; corrections of the semi-normal refinement {f['sizes']}")
    assert f["last"] < 1e-15 and len(f["sizes"]) <= 6


@pytest.mark.parametrize("key", dr.KEYS, ids=IDS)
def test_floor_is_the_written_constant(ref, key):
    f = ref(*key)
    print(f"case {key[0]}, lambda {key[1]:g}: S measured {f['S']:.3e} (written {dr.S[key]:.2e}, bar {dr.bar(*key):.2e}): "
          + ", ".join(f"{k} {v:.3e}" for k, v in f["errs"].items()))
    assert f["S"] <= dr.S[key] <= 1.25 * f["S"]


@pytest.mark.parametrize("lam", dr.LAMBDAS)
@pytest.mark.parametrize("name", dr.LADDER_CASES)
def test_elimination_order_is_no_term_of_its_own(oracle, ref, name, lam):
    """dense Cholesky of the SAME matrix with the keyframes eliminated in natural order (the one-wave sweeps), reversed, from
    both ends towards the middle (the two-sided sweep) and with one separator last (the partitioned solve): each at or below
    4 x S.  No form is owed a bar of its own."""
    f = ref(name, lam)
    H, g = rr.normal_equations(oracle, f["case"])
    D = rr.band_dense(H)
    for what, order in dr.orders(f["case"].n).items():
        assert sorted(order) == list(range(f["case"].n))
        e = rr.err(dr.dense_solve_in_order(D, g, lam, order), f["dref"])
        print(f"case {name}, lambda {lam:g}, {what}: {e:.3e} = {e / dr.S[(name, lam)]:.2f} x S")
        assert e <= 4.0 * dr.S[(name, lam)], what


@pytest.mark.parametrize("key", dr.KEYS, ids=IDS)
def test_the_bar_can_fail(oracle, ref, key):
    """every mutation of direct_ref.mutations lands beyond 10 x the bar: a condition on the INPUTS.  Between factors: all that
    do not touch the X0 prior's keyframe, but for direct_ref.LEFT_OUT (at most one per case) and direct_ref.CAP_NOT_MET"""
    name, lam = key
    f = ref(*key)
    case, b = f["case"], dr.bar(*key)
    muts = dr.mutations(oracle, case, f["rows"], lam)
    kinds = {what for what, _, _ in muts}
    want = {"bias columns of the last IMU factor dropped"}
    prior = 0 if case.prior_k is not None else None
    tested = {fac for _, fac, _ in muts if fac is not None}
    assert tested == {(a, b_) for _, a, b_, _, _ in f["rows"].find("btw") if prior not in (a, b_)}
    assert tested or case.n <= 3                 # (n = 2 has no between factor, n = 3 none off the X0 prior's keyframe)
    if tested:
        want |= {"between factor's cross block dropped from H", "between factor dropped from H only", "between factor dropped from g only"}
    if lam == 1.0:
        want |= {"lambda missing everywhere"} | ({"lambda missing on the middle keyframe", "lambda doubled on the middle keyframe"} if case.n >= 3 else set())
    want |= {"marginal prior's rows of keyframe lo + 2 dropped"} if case.marg is not None else {"X0 prior's rows dropped"}
    want |= {"a block of the last far factor dropped"} if case.far is not None else set()
    assert kinds == want
    weakest, weak = {}, {}
    for what, fac, x in muts:
        m = rr.err(x, f["dref"]) / b
        if fac is None:
            print(f"case {name}, lambda {lam:g}, {what}: {m:.3g} x the bar")
            assert m > 10.0, what
        else:
            weakest[what] = min(weakest.get(what, (np.inf, None)), (m, fac))
            if not m > 10.0:
                weak.setdefault(fac, []).append((what, m))
    for what, (m, fac) in weakest.items():
        print(f"case {name}, lambda {lam:g}, {what}: {len(tested)} factors, the weakest {fac} at {m:.3g} x the bar")
    for fac, w in weak.items():
        print(f"case {name}, lambda {lam:g}, NOT beyond 10 x the bar, factor {fac}: " + ", ".join(f"{what} {m:.3g}" for what, m in w))
    if name in dr.CAP_NOT_MET:
        return
    assert set(weak) <= ({dr.LEFT_OUT[name]} if name in dr.LEFT_OUT else set()), weak


def test_at_most_one_between_factor_is_left_out_per_case():
    assert all(isinstance(f, tuple) and len(f) == 2 and isinstance(f[0], int) for f in dr.LEFT_OUT.values())
    assert set(dr.LEFT_OUT) <= {c for c, _ in dr.KEYS} and not set(dr.LEFT_OUT) & set(dr.CAP_NOT_MET)


def test_lambda_is_blind_at_the_default(oracle, ref):
    """why the lambda = 1 cases exist: at lambda = 1e-5 the three damping mutations move the increment by about the bar or
    less from n = 9 on -- direct_ref.LAMBDA_BLIND records the largest multiples"""
    worst = [0.0, 0.0, 0.0]
    for name in dr.BATCH_CASES:
        f = ref(name, rr.LAMBDA)
        if f["case"].n < 9:
            continue
        for i, (what, x) in enumerate(dr.blind_lambda_mutations(oracle, f["case"], f["rows"], rr.LAMBDA).items()):
            m = rr.err(x, f["dref"]) / dr.bar(name, rr.LAMBDA)
            worst[i] = max(worst[i], m)
            print(f"case {name}, lambda 1e-05, {what}: {m:.3g} x the bar")
    print(f"largest: {worst} (written {dr.LAMBDA_BLIND})")
    for w, written in zip(worst, dr.LAMBDA_BLIND):
        assert w <= written <= 1.5 * w + 0.1 and written < 20.0
