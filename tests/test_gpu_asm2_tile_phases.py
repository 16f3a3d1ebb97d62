"""-m gpu: the two-wave assembling sweep (k_band_forward_asm2) against the one-wave assembling sweep (k_band_forward_asm) where
the eliminator's J-tile switch falls in different phases of its four-times unrolled step loop.

The eliminator wave asks for the assembler's progress with an LDS read it does not wait for, uses the answer behind the wait
that follows the panel's LDS writes, and puts the next J tile in place in the step in which factor k + 6 opens a tile -- a step
whose phase (k & 3) depends on the window's first slot.  Both sweeps issue the same arithmetic row by row, so everything they
leave is identical bit for bit.  Six windows of 5, 9, 16, 23, 33 and 41 keyframes (shorter than a tile, than two, not a
multiple of the unroll; the three longest cross three, four and five tile boundaries) whose first slots have lo & 7 = 0, 3
and 7; 4 LM trials, then two marginalised slides (each moves every first slot on by one) with 4 trials behind each."""
import numpy as np
import pytest

from tests.test_gpu_ingest import _engine
from vil_sensor_fusion_amd import synth
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS

pytestmark = pytest.mark.gpu
LENGTHS = (5, 9, 16, 23, 33, 41)
FIRST = (3, 7, 0, 7, 3, 0)       # lo & 7 of the three short and of the three long windows: 3, 7, 0 each
N = 56                           # keyframes resident per window: the slides find their factors there
TRIALS, SLIDES = 4, 2


def _run(seqs, waves):
    eng = _engine(None, seqs, N, 0, solve_assemble_min=1, sweep_two_sided_max=0, chunks=1, solve_assemble_waves=waves)
    for w, (lo, m) in enumerate(zip(FIRST, LENGTHS)):
        eng.set_prior(w, lo, synth.prior_record(seqs[w].gt_states[lo], REFERENCE_PRIOR_SIGMAS))
        eng.set_range(w, lo, lo + m)
    assert eng.solve_form() == "assembling"
    out = []
    for u in range(SLIDES + 1):
        if u:
            eng.slide(REFERENCE_PRIOR_SIGMAS, marginalize=True)
        eng.iterate(TRIALS)
        out.append([(eng.get_states(w, lo + u, m), eng.read_delta(w, lo + u, m), eng.read_lm(w))
                    for w, (lo, m) in enumerate(zip(FIRST, LENGTHS))])
    eng.close()
    return out


def test_two_wave_sweep_gives_the_bits_of_the_one_wave_sweep_at_every_tile_phase():
    assert {lo & 7 for lo in FIRST[:3]} == {lo & 7 for lo in FIRST[3:]} == {0, 3, 7}
    for lo, m in zip(FIRST[3:], LENGTHS[3:]):       # tile boundaries strictly inside (lo, lo + m)
        assert (lo + m - 1) // 8 - lo // 8 >= 3
    seqs = [synth.make_sequence(seed=940 + i, n_kf=N + 2) for i in range(len(LENGTHS))]
    one, two = _run(seqs, 1), _run(seqs, 2)
    for u in range(SLIDES + 1):
        for w in range(len(LENGTHS)):
            (sa, da, la), (sb, db, lb) = one[u][w], two[u][w]
            assert la["solve_failures"] == 0 and la["accepted"] > 0, (u, w, la)
            assert np.isfinite(sa).all() and np.abs(da).max() > 0.0, (u, w)
            np.testing.assert_array_equal(sa, sb, err_msg=f"states, slide {u}, window {w}")
            np.testing.assert_array_equal(da, db, err_msg=f"increments, slide {u}, window {w}")
            assert la == lb, (u, w, la, lb)
