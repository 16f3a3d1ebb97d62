"""The cases of tests/test_gpu_robust_far.py have teeth: conditions on tests/robust_far_ref.py's cases, checked on the CPU.

  (a) S -- the largest position difference between three correct host optimisers over ALL nine (loss, window) cases -- is below
      1e-6 m, BASELINE's bar on positions;
  (b) the Gaussian optimum of every case is at least 1000 bars (16 S) from the robust one: an engine that ignores the far losses
      fails the optimum test;
  (c) the outlier closure's weight at the optimum is below 0.1, the other closures' above 0.99;
  (d) the losses put on the NEXT entry of the list move the optimum by more than 10 bars: a loss that lands on the wrong entry
      fails it too;
  (e) the robust optimum is closer to the clean data's optimum than the Gaussian one is.
A case that does not satisfy them is to be changed; the factor is not."""
import numpy as np
import pytest

from tests import robust_far_ref as F
from tests import robust_ref as R


def test_the_optimiser_is_robust_refs():
    assert F._optimise.__code__ is R.optimise.__code__
    assert F._optimise.__globals__["robust_rows"] is F.robust_rows and F._optimise.__globals__["cost"] is F.cost


def test_S_is_below_the_baseline_bar():
    S = F.S_all()
    for loss in R.LOSSES:
        print(f"{R.NAMES[loss]}: S per window {[F.optima(loss, w)['S'] for w in range(F.B)]}")
    print(f"S over the nine cases {S:.3e} m, the bar 16 S = {16 * S:.3e} m")
    assert 0.0 < S < 1e-6, S


@pytest.mark.parametrize("loss", R.LOSSES)
def test_optimum_cases_have_teeth(oracle, loss):
    bar = 16 * F.S_all()
    for w in range(F.B):
        o, c = F.optima(loss, w), F.opt_cases(loss)[w]
        d = R.position_error(o["gauss"], o["irls"])
        sh = R.position_error(o["shifted"], o["irls"])
        wg = F.far_weights(oracle, c, o["irls"], c["loss"], c["k"])
        rc, gc = R.position_error(o["irls"], o["clean"]), R.position_error(o["gauss"], o["clean"])
        print(f"{R.NAMES[loss]} window {w}: S {o['S']:.2e}; Gaussian optimum {d:.3e} m away = {d / bar:.3g} bars; losses on the next entry "
              f"{sh:.3e} m = {sh / bar:.3g} bars; weights {[f'{x:.3g}' for x in wg]}; from the clean optimum: robust {rc:.2e} m, Gaussian {gc:.2e} m")
        assert d >= 1000 * bar
        assert sh > 10 * bar
        assert wg[0] < 0.1 and all(x > 0.99 for x in wg[1:]), wg
        assert rc < gc
        # a mix in every list, every lossy entry with a k of its own, pairs the band cannot hold
        assert list(c["loss"]) == [loss, loss, R.NONE] and c["k"][0] != c["k"][1]
        a, b, _ = c["far"]
        assert [(int(x), int(y)) for x, y in zip(a, b)] == list(F.PAIRS)


def test_linearisation_cases_cover_the_plan(oracle):
    cases = F.lin_cases()
    seen = set()
    for c in cases:
        a, b, rec = c["far"]
        assert a.size == 9 and (c["loss"] == R.NONE).any() and len(set(c["loss"])) == 4
        ks = [k for k, l in zip(c["k"], c["loss"]) if l != R.NONE]
        assert len(set(ks)) == len(ks)                        # every k distinct
        for f in range(a.size):
            r, _, _ = oracle.between_factor(rec[f], c["states"][a[f]], c["states"][b[f]])
            ratio = c["ratio"][f]
            if ratio is None:
                assert not r.any()
            seen.add((int(c["loss"][f]), "zero" if ratio is None else "inside" if ratio < 0.9 else "at" if ratio < 1.5 else
                      "huge" if ratio >= 1e5 else "outside"))
    for loss in R.LOSSES:
        assert {(loss, x) for x in ("zero", "inside", "at", "outside", "huge")} <= seen, (loss, seen)
