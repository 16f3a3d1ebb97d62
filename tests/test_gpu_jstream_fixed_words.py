"""-m gpu: the words of the J stream that belong to the record, not to the states.

Of the 291 entries of an IMU factor's whitened Jacobian that are not structurally zero, 90 are the same at every state:
X_j.p (columns 12..14) is -R(:, 3..5) and B_j (columns 24..29) is -R(:, 9..14) of the record's square-root information
R (words 70..189 of the record, upper triangle packed by rows).  K1 does not write them: they are put into BOTH buffers
of the J stream when the record is written (K0, vf_engine_set_imu, vf_engine_grow) and only moved after that
(vf_engine_compact).  Every road a record can take is walked here, at the smallest shape that can go wrong: 2 windows
of capacity 64 with 21 keyframes -- 20 factors, three J tiles of 8 slots, the last one partial -- one window starting at
slot 0, the other at slot 3 after three vf_engine_drop_oldest.  (vf_engine_compact moves whole tiles of 64 slots, so
its case needs the windows at slot 64 of a capacity of 128.)

After every step, for both buffers (read_imu_lin which = 0 and 1):
  the 90 fixed entries   ==  the negated words of the record get_imu returns (exact: a copy with the sign flipped)
  the 159 structural zeros == 0
  the other 201 entries  agree with the oracle's Jacobian at the states of that buffer to 1e-12 of the block's largest
                         entry, the bar of tests/test_gpu_parity.py
Where a step does not linearise by itself (a record has just been written), the fixed entries are checked before any
linearisation runs -- they must be there already -- and everything after linearize(0) and linearize(1)."""
import numpy as np
import pytest

from tests import helpers
from vil_sensor_fusion_amd import Engine, EngineOpts, synth
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS

pytestmark = pytest.mark.gpu

N = 21                # keyframes of a window: factors in slots 1..20
LO1 = 3               # first keyframe of window 1
TOL = 1e-12           # tests/test_gpu_parity.py, residuals / Jacobians
SWEEP = dict(chunks=1, sweep_two_sided_max=0)

ROW, COL = np.meshgrid(np.arange(15), np.arange(30), indexing="ij")
FIXED = ((COL >= 12) & (COL < 15) & (ROW <= COL - 9)) | ((COL >= 24) & (ROW <= COL - 15))
ZERO = ((COL < 18) & (ROW >= 9)) | ((COL >= 3) & (COL < 6) & (ROW >= 6)) | ((COL >= 12) & (COL < 15) & (ROW > COL - 9)) | \
       ((COL >= 18) & (COL < 24) & (ROW > COL - 9)) | ((COL >= 24) & (ROW > COL - 15))
REST = ~FIXED & ~ZERO
assert FIXED.sum() == 90 and ZERO.sum() == 159 and REST.sum() == 201


@pytest.fixture(scope="module")
def problems(oracle):
    """two sequences of N + 3 keyframes: records by the oracle, perturbed initial values (computed once, never changed)"""
    seqs = [synth.make_sequence(seed=940 + w, n_kf=N + 3) for w in range(2)]
    return seqs, [helpers.build_problem(oracle, s, perturb=0.01) for s in seqs]


def _engine(problems, records, base=0, capacity=64, states=None, **opts):
    """window 0 on [base, base + N), window 1 on [base + 3, base + N) after three drop_oldest; records from K0 or set_imu"""
    seqs, probs = problems
    eng = Engine(EngineOpts(windows=2, capacity=capacity, **opts))
    for w, (seq, p) in enumerate(zip(seqs, probs)):
        eng.set_states(w, base, (p["states"] if states is None else states[w])[:N])
        if records == "k0":
            eng.preintegrate(w, base + 1, seq.imu_off[1:N + 1], seq.imu_steps, np.zeros(6), synth.CARLA_IMU_COV)
        else:
            eng.set_imu(w, base + 1, p["imu"][1:N])
        m = seq.btw_b < N
        eng.set_between(w, seq.btw_a[m] + base, seq.btw_b[m] + base, synth.between_records(seq)[m])
        lo = base + (LO1 if w else 0)
        eng.set_prior(w, lo, synth.prior_record(p["states"][lo - base], REFERENCE_PRIOR_SIGMAS))
        eng.set_range(w, base, base + N)
    for _ in range(LO1):
        eng.drop_oldest()
    eng.set_range(0, base, base + N)
    return eng


def _check(eng, oracle, problems, ranges, what, full=True):
    """the three properties for every factor of every window, both buffers; ranges[w] = (lo, hi)"""
    worst = 0.0
    for w, (lo, hi) in enumerate(ranges):
        n = hi - lo - 1
        rec = eng.get_imu(w, lo + 1, n)
        for which in (0, 1):
            _, J = eng.read_imu_lin(w, lo + 1, n, which=which)
            st = (eng.get_estimate if which else eng.get_states)(w, lo, hi - lo) if full else None
            for f in range(n):
                R = np.zeros((15, 15))
                R[np.triu_indices(15)] = rec[f, 70:190]
                E = np.zeros((15, 30))
                E[:, 12:15], E[:, 24:30] = -R[:, 3:6], -R[:, 9:15]
                assert np.all(np.diag(R) > 0), "slot without a record: nothing would be checked"
                assert np.array_equal(J[f][FIXED], E[FIXED]), (what, "fixed words", w, which, lo + 1 + f)
                if not full:
                    continue
                assert not J[f][ZERO].any(), (what, "structural zeros", w, which, lo + 1 + f)
                _, Jo = oracle.imu_factor(rec[f], problems[1][w]["gravity"], st[f], st[f + 1])
                err = np.abs(J[f] - Jo)[REST].max() / np.abs(Jo).max()
                worst = max(worst, err)
                assert err < TOL, (what, "state-dependent entries", w, which, lo + 1 + f, err)
    if full:
        print(f"{what}: state-dependent entries vs the oracle, worst relative error {worst:.2e}")


def _check_cold(eng, oracle, problems, ranges, what):
    """a record has just been written: its words are in the stream already; the rest after a linearisation of each buffer"""
    _check(eng, oracle, problems, ranges, what + " (before any linearisation)", full=False)
    eng.linearize(0)
    eng.linearize(1)
    _check(eng, oracle, problems, ranges, what)


RANGES = [(0, N), (LO1, N)]
FAR_OFF = np.array([1.5, 1.5, -1.5, 20, -20, 10, 10, -10, 5, 0.5, 0.5, 0.5, 0.1, 0.1, 0.1])      # tangent of a state: theta, p, v, biases


def test_a_preintegrate_then_linearize(oracle, problems):
    eng = _engine(problems, "k0")
    _check_cold(eng, oracle, problems, RANGES, "K0")
    eng.close()


def test_b_ingest_tail_slide_and_the_tail_linearisation(oracle, problems):
    """the TAIL form of K0 writes slot hi; the warm solve that follows linearises that slot alone in the current buffer
    (k_linearize_tail), everything in the trial buffer"""
    from tests.test_gpu_ingest import _feed
    eng = _engine(problems, "k0", **SWEEP)
    eng.iterate(4)
    eng.ingest_tail(*_feed(problems[0], N))
    eng.slide(REFERENCE_PRIOR_SIGMAS, marginalize=True)
    eng.iterate(1)
    eng.ingest_status()
    _check(eng, oracle, problems, [(1, N + 1), (LO1 + 1, N + 1)], "ingest_tail + slide + iterate(1)")
    eng.close()


def test_c_records_put_in_with_set_imu(oracle, problems):
    eng = _engine(problems, "set")
    _check_cold(eng, oracle, problems, RANGES, "set_imu")
    eng.close()


@pytest.mark.parametrize("records", ["k0", "set"])
def test_d_grow(oracle, problems, records):
    """the records come over, the J stream does not: vf_engine_grow writes the fixed words of every record again"""
    eng = _engine(problems, records)
    eng.linearize(0)
    eng.grow(128)
    _check_cold(eng, oracle, problems, RANGES, "grow")
    eng.close()


def test_e_compact(oracle, problems):
    """both buffers of the J stream move with the records, whole tiles of 64 slots"""
    eng = _engine(problems, "k0", base=64, capacity=128)
    eng.linearize(0)
    eng.linearize(1)
    eng.compact(64)
    _check(eng, oracle, problems, RANGES, "compact")
    _check_cold(eng, oracle, problems, RANGES, "compact, linearised again")
    eng.close()


def test_f_a_slot_preintegrated_again_with_another_bias(oracle, problems):
    """slots 9 (inside the second tile) and 20 (the partial third) of both windows, another bias estimate: the record changes,
    and with it the fixed words of both buffers, at once"""
    seqs, _ = problems
    eng = _engine(problems, "k0")
    eng.linearize(0)
    eng.linearize(1)
    for w, seq in enumerate(seqs):
        for k in (9, N - 1):
            before = eng.get_imu(w, k, 1)[0]
            steps = seq.imu_steps[seq.imu_off[k]:seq.imu_off[k + 1]]
            eng.preintegrate(w, k, np.array([0, len(steps)]), steps, np.array([0.05, -0.04, 0.03, 0.02, -0.01, 0.015]), synth.CARLA_IMU_COV)
            after = eng.get_imu(w, k, 1)[0]
            # (enough of the 120 words differ for the check below to tell the new record's words from the old one's)
            assert np.count_nonzero(after[70:] != before[70:]) >= 60, "the second preintegration left the square-root information as it was"
    _check_cold(eng, oracle, problems, RANGES, "second preintegration")
    eng.close()


def test_g_trials_with_a_rejection_keep_the_fixed_words(oracle, problems):
    """three LM trials from a start with keyframe 10 far off.  Window 0, 1.2 rad / 16 m / 8 m/s off: every trial is rejected (on the
    CPU oracle all three, from 0.64 of FAR_OFF on), so the trial buffer is linearised three times at three other states.  Window
    1, half as far: every trial is accepted (on the oracle up to 0.62 of FAR_OFF) and the buffers change places each time.  The
    fixed words are in whichever buffer is read.  Trial counts as in the two-kernel form (K3 + band solve: the same Jacobians,
    other sums), states to rounding (1e-9, the bar of tests/test_gpu_assembling_sweep.py)."""
    _, probs = problems
    states = [p["states"].copy() for p in probs]
    for s, scale in zip(states, (0.8, 0.4)):
        s[10] = oracle.retract(s[10], scale * FAR_OFF)
    two = _engine(problems, "k0", states=states, solve_assemble_min=0, **SWEEP)
    asm = _engine(problems, "k0", states=states, solve_assemble_min=1, **SWEEP)
    assert two.solve_form() == "one_wave" and asm.solve_form() == "assembling"
    for e in (two, asm):
        e.iterate(3)
    for w, (lo, hi) in enumerate(RANGES):
        a, b = two.read_lm(w), asm.read_lm(w)
        print(f"window {w}: two-kernel form {a}, assembling sweep {b}")
        assert (a["accepted"], a["rejected"], a["solve_failures"]) == (b["accepted"], b["rejected"], b["solve_failures"])
        assert a["accepted"] + a["rejected"] == 3
        assert b["accepted" if w else "rejected"] >= 1, "the start does not do what it is here for"
        assert np.abs(two.get_states(w, lo, hi - lo) - asm.get_states(w, lo, hi - lo)).max() <= 1e-9
    for e, what in ((two, "iterate(3), two-kernel form"), (asm, "iterate(3), assembling sweep")):
        _check(e, oracle, problems, RANGES, what)
        e.close()
