"""-m gpu: the two forms of the back substitution behind a split or assembling forward sweep (vf_engine_tuning.solve_backsub_form).

k_band_backward (form 1) is built for two waves per SIMD: one set of column registers, two panels in flight, the recursion not
software-pipelined.  k_band_backward_1w (form 2) is the kernel for batches of at most one window per SIMD: the pipelined loop of
the fused kernel, two column-register sets, four panels in flight.  Both do the same arithmetic in the same order on the same
panels, so increments and states are identical bit for bit.  Windows of 4, 5, 7 and 34 keyframes: the padded length equal to the
prefetch depth (4: every panel is loaded before the loop and every later load is past the window's head), lengths that are no
multiple of four (identity pads behind the last real keyframe), and a window of several turns of the four-step loop."""
import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_ingest import _engine
from vil_sensor_fusion_amd import Engine, EngineOpts, synth

pytestmark = pytest.mark.gpu
LENGTHS = (4, 5, 7, 34)
N = 40
FORWARD = {"split": dict(solve_split_min=1, solve_assemble_min=0), "assembling": dict(solve_split_min=0, solve_assemble_min=1)}


@pytest.fixture(scope="module")
def seqs():
    return [synth.make_sequence(seed=960 + i, n_kf=N + 2) for i in range(len(LENGTHS))]


def _run(seqs, forward, form):
    eng = _engine(None, seqs, N, 0, chunks=1, sweep_two_sided_max=0, solve_backsub_form=form, **FORWARD[forward])
    for w, m in enumerate(LENGTHS):
        eng.set_range(w, 0, m)
    assert eng.solve_form() == ("one_wave_split" if forward == "split" else "assembling")
    out = []
    for _ in range(3):
        eng.iterate(1)
        out.append([(eng.read_delta(w, 0, m), eng.get_states(w, 0, m), eng.read_lm(w)) for w, m in enumerate(LENGTHS)])
    eng.close()
    return out


@pytest.mark.parametrize("forward", ["split", "assembling"])
def test_both_forms_give_the_same_bits(seqs, forward):
    one, two = _run(seqs, forward, 1), _run(seqs, forward, 2)
    by_batch = _run(seqs, forward, 0)          # (four windows: at most one per SIMD on any device, i.e. form 2 by the plan's rule)
    for t in range(3):
        for w in range(len(LENGTHS)):
            (da, sa, la), (db, sb, lb), (dc, sc, lc) = one[t][w], two[t][w], by_batch[t][w]
            assert la["solve_failures"] == 0 and np.abs(da).max() > 0.0 and np.isfinite(sa).all(), (forward, t, w, la)
            np.testing.assert_array_equal(da, db, err_msg=f"increments, {forward}, trial {t}, window {w}")
            np.testing.assert_array_equal(sa, sb, err_msg=f"states, {forward}, trial {t}, window {w}")
            np.testing.assert_array_equal(da, dc)
            np.testing.assert_array_equal(sa, sc)
            assert la == lb == lc, (forward, t, w)


def test_incremental_engine_is_unchanged(oracle):
    """An incremental engine substitutes back with its own kernel (k_inc_backward, the two-per-SIMD form's loop with the early
    stop) and takes the split sweep for its whole-window updates: whichever form that sweep's back substitution has, linearisation
    points, estimates and increments of every update are the same."""
    n0, n = 30, 48
    seq = synth.make_sequence(seed=97, n_kf=n)
    prob = helpers.build_problem(oracle, seq, perturb=0.003)
    opts = dict(windows=1, capacity=n + 8, chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, solve_split_min=1,
                refine_iterations=0, lm_excursion=0, incremental=1)
    engs = [Engine(EngineOpts(solve_backsub_form=form, **opts)) for form in (1, 2, 0)]
    for e in engs:
        helpers.load_engine(e, 0, prob, 0, n0)
    hi = n0
    for u in range(7):
        for e in engs:
            e.isam_step(1e-4)
        for e in engs[1:]:
            np.testing.assert_array_equal(e.get_states(0, 0, hi), engs[0].get_states(0, 0, hi))
            np.testing.assert_array_equal(e.get_estimate(0, 0, hi), engs[0].get_estimate(0, 0, hi))
            np.testing.assert_array_equal(e.read_delta(0, 0, hi), engs[0].read_delta(0, 0, hi))
            assert e.incremental_info(0) == engs[0].incremental_info(0)
        hi += 1 + u % 3
        for e in engs:
            e.set_range(0, 0, hi)
    assert engs[0].incremental_info(0)["updates"] >= 5
    for e in engs:
        e.close()
