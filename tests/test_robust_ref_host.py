"""The cases of tests/test_gpu_robust.py have teeth: a condition on tests/robust_ref.py's cases, checked on the CPU.

  (a) the Gaussian optimum and the robust optimum of every optimum case differ by at least 1000 x the bar of the optimum test, so a
      kernel that ignores the loss fails it;
  (b) replacing J^ by alpha J (gamma dropped) moves the linearisation of every robust outlier of the linearisation cases by at least
      100 x the bar of the linearisation test;
  (c) so does replacing (r^, J^) by GTSAM's (sqrt(w) r, sqrt(w) J).
A case that does not satisfy all three is to be changed; the factor is not."""
import numpy as np
import pytest

from tests import robust_ref as R


@pytest.mark.parametrize("loss", R.LOSSES)
def test_optimum_cases_have_teeth(loss):
    S = max(R.optima(loss, w)["S"] for w in range(R.B))
    assert S < 1e-6, S
    for w in range(R.B):
        o, c = R.optima(loss, w), R.opt_cases(loss)[w]
        d = R.position_error(o["gauss"], o["irls"])
        print(f"{R.NAMES[loss]} window {w}: S {o['S']:.2e} (largest {S:.2e}), Gaussian optimum {d:.3e} m from the robust one = {d / (16 * S):.3g} bars")
        assert d >= 1000 * 16 * S
        assert c["loss"][c["bad"]] == loss and (c["loss"] == R.NONE).any() and (c["loss"] == loss).sum() >= 2    # a mix in every window
        # the outlier IS one: its weight at the optimum is far below 1, the others' is not
        from vil_sensor_fusion_amd import robust
        rw = R._rows(__import__("oracle.oracle", fromlist=["oracle"]), c["prob"], o["irls"])
        for f, row0 in R._btw_blocks(c["prob"], rw):
            s = float(np.linalg.norm(rw.r[row0:row0 + 6]))
            wgt = robust.weight(int(c["loss"][f]), c["k"][f], s)
            assert (wgt < 0.2) == (f == c["bad"]), (f, s, wgt)


def test_linearisation_cases_have_teeth(oracle):
    cases = R.lin_cases()
    assert len(cases) == R.B
    seen, dists = set(), set()
    worst_S, figures = 0.0, []
    for w, c in enumerate(cases):
        p = c["prob"]
        assert (c["loss"] == R.NONE).any() and len(set(c["loss"])) == 4            # every loss and a Gaussian factor in every window
        for f, (a, b, rec) in enumerate(zip(p["btw_a"], p["btw_b"], p["btw"])):
            r, Ja, Jb = oracle.between_factor(rec, c["states"][a], c["states"][b])
            J, loss, k, ratio = np.hstack([Ja, Jb]), int(c["loss"][f]), float(c["k"][f]), c["ratio"][f]
            dists.add(int(b - a))
            seen.add((loss, "zero" if ratio is None else "inside" if ratio < 0.9 else "at" if ratio < 1.5 else "huge" if ratio >= 1e5 else "outside"))
            if ratio is None:
                assert not r.any()                                                  # r = 0 exactly
            if not R.near_threshold(loss, ratio):
                worst_S = max(worst_S, R.hat_S(r, J, loss, k))
            if loss != R.NONE and ratio is not None and ratio >= 3.0:
                figures.append((w, f, loss, ratio, r, J, k))
    assert dists >= {1, 3}
    for loss in R.LOSSES:
        assert {(loss, x) for x in ("inside", "at", "outside", "huge")} <= seen, (loss, seen)
    assert any(x == "zero" for _, x in seen)
    assert len(figures) >= 9
    bar = 16 * worst_S
    for w, f, loss, ratio, r, J, k in figures:
        want = R.mp_hat(r, J, loss, k)
        al = float(want[2])
        dropped = R.hat_error(al * r, al * J, r, J, loss, k, want)                  # (b) gamma dropped
        gr, gJ = R.gtsam_form(r, J, loss, k)
        gtsam = R.hat_error(gr, gJ, r, J, loss, k, want)                            # (c) GTSAM's form
        print(f"window {w} factor {f} {R.NAMES[loss]} s/k {ratio:g}: gamma dropped {dropped / bar:.3g} bars, GTSAM's form {gtsam / bar:.3g} bars (bar {bar:.2e})")
        assert dropped >= 100 * bar and gtsam >= 100 * bar
