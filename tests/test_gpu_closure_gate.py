"""-m gpu: the loop-closure gate (vf_engine_gate_closures, kernels/kclosure.inc; vf_gate_closure) against the references of
tests/closure_ref.py, whose numbers tests/test_closure_ref_host.py fixes on the CPU.

The windows are those of tests/cov_ref.py (at most 56 keyframes loaded), engines and loading those of
tests/test_gpu_marginals_small.py.  Every candidate of a window is gated twice, with a consistent and a gross measurement
(gate_ref.measurement), in two calls of at most four candidates per window.  For each:
    Sigma_J within 16 x S_JOINT[case] of the extended-precision reference (closure_ref.err_joint),
    nis within closure_ref.NIS_BAR (relative) of mpmath fed the DEVICE's Sigma_J,
    xi within XI_BAR per component, nis_measurement within closure_ref.measurement_bar.
No LM trial runs before a call unless the test says so: the states read back are the bits that were loaded."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_direct_small.py)

from tests import closure_ref as cl
from tests import cov_ref as cr
from tests import refine_ref as rr
from tests.test_gpu_direct_small import BATCH_CAPACITY, device_marg_case, load, make_engine
from tests.test_gpu_marginals_small import FACTORINGS
from vil_sensor_fusion_amd import _lib
from vil_sensor_fusion_amd._lib import VilFusionError

pytestmark = pytest.mark.gpu
_refs, _runs = {}, {}
THRESHOLD = _lib.CHI2_6_99
NO_REC = np.concatenate([[1.0], np.zeros(6), np.ones(21)])


@pytest.fixture(scope="module")
def ref(oracle):
    """(case, rows and Sigma_ref as cov_ref.reference names them; closure_ref.reference without the floors and the CPU's own nis,
    which tests/test_closure_ref_host.py is for) of a case, built once"""
    def get(name):
        if name not in _refs:
            _refs[name] = reference(oracle, cr.make_case(oracle, name))
        return _refs[name]
    return get


def reference(oracle, case):
    rw = rr.rows(oracle, case)
    Sref, last, _ = cr.exact_cov(rw)
    assert cl.S_JOINT[case.name] is None or last <= cl.S_JOINT[case.name] / 100.0
    f = dict(case=case, rows=rw, Sref=Sref)
    return f, cl.reference(oracle, f, nis=False, floors=False)[0]


def gate_cases(eng, cases, crefs, threshold=THRESHOLD):
    """every candidate of cl.candidates(case) of window w = index of the case, once per kind: {(w, (a, b), kind): (record dict, Sigma_J)}.
    A candidate that cannot be tested (L1's) goes in with a record that is never read"""
    out = {}
    for kind in cl.KINDS:
        ws, a, b, recs = [], [], [], []
        for w, (case, cref) in enumerate(zip(cases, crefs)):
            for c in cl.candidates(case):
                ws.append(w), a.append(c[0]), b.append(c[1])
                recs.append(cref[c]["recs"][kind] if c in cref else NO_REC)
        got = eng.gate_closures(ws, a, b, np.array(recs), threshold=threshold)
        status, nis = eng.read_closure_gate_all(len(ws))
        for i, g in enumerate(got):
            assert (g["window"], g["a"], g["b"]) == (ws[i], a[i], b[i])
            assert _lib.GATE_STATUS[status[i]] == g["status"] and (nis[i] == g["nis"] or (np.isnan(nis[i]) and np.isnan(g["nis"])))
            out[(ws[i], (a[i], b[i]), kind)] = (g, eng.read_closure_joint(i))
    return out


def check(name, case, cref, got, w, what):
    """every candidate of one window against the bars; returns the worst multiples (Sigma_J, nis)"""
    worst = [0.0, 0.0]
    for (a, b), c in cref.items():
        for kind in cl.KINDS:
            g, SJ = got[(w, (a, b), kind)]
            assert g["status"] == "ok", (name, a, b, kind, g)
            e = cl.err_joint(SJ, c["SJ"])
            m = cl.nis_mp(c["recs"][kind], None, None, SJ, c["factor"][kind])
            en = abs(g["nis"] - m["nis"]) / m["nis"]
            ex = float(np.max(np.abs(g["xi"] - m["xi"])))
            em = abs(g["nis_measurement"] - m["nis_measurement"])
            print(f"case {name}, {what}, ({a}, {b}) {kind:10s}: Sigma_J error {e:.3e} = {e / cl.bar(name):.3f} of the bar {cl.bar(name):.2e}; nis {g['nis']:.6e} "
                  f"rel. error {en:.2e} = {en / cl.NIS_BAR:.3f} of the bar; xi {ex:.1e}; nis_measurement {em:.1e} (bar {cl.measurement_bar(c['recs'][kind], m['nis_measurement']):.1e})")
            assert np.array_equal(SJ, SJ.T)
            assert e <= cl.bar(name), (name, what, a, b)
            assert en <= cl.NIS_BAR, (name, what, a, b, kind)
            assert ex <= cl.XI_BAR and em <= cl.measurement_bar(c["recs"][kind], m["nis_measurement"]), (name, what, a, b, kind)
            assert g["rejected"] == (m["nis"] > THRESHOLD) == (kind == "gross")
            worst = [max(worst[0], e / cl.bar(name)), max(worst[1], en / cl.NIS_BAR)]
    return worst


def same_bits(x, y):
    assert set(x) == set(y)
    for k in x:
        (g, S), (h, T) = x[k], y[k]
        np.testing.assert_array_equal(S, T)
        np.testing.assert_array_equal(g["xi"], h["xi"])
        assert (g["status"], g["rejected"]) == (h["status"], h["rejected"]), k
        assert np.array_equal([g["nis"], g["nis_measurement"]], [h["nis"], h["nis_measurement"]], equal_nan=True), k


def run_batch(ref, factor):
    """every ladder and offset case as one window each of ONE engine, every candidate of closure_ref on it"""
    if factor not in _runs:
        kw, form = FACTORINGS[factor]
        cases = [ref(name)[0]["case"] for name in cr.BATCH_CASES]
        eng = make_engine(len(cases), BATCH_CAPACITY, rr.LAMBDA, **kw)
        assert eng.solve_form() == form
        for w, c in enumerate(cases):
            load(eng, w, c, BATCH_CAPACITY)
        _runs[factor] = gate_cases(eng, cases, [ref(name)[1] for name in cr.BATCH_CASES])
        for w, c in enumerate(cases):
            n = min(c.prob["n"], BATCH_CAPACITY)
            np.testing.assert_array_equal(eng.get_states(w, 0, n), c.states[:n])
        eng.close()
    return _runs[factor]


# ---------------------------------------------------------------- 1. the three factorings
@pytest.mark.parametrize("factor", FACTORINGS)
def test_every_factoring(ref, factor):
    got = run_batch(ref, factor)
    assert max(len(cl.candidates(ref(n)[0]["case"])) for n in cr.BATCH_CASES) == _lib.CLOSURE_GATE_MAX
    for w, name in enumerate(cr.BATCH_CASES):
        f, cref = ref(name)
        check(name, f["case"], cref, got, w, f"factor = {factor}")
    for kind in cl.KINDS:                                     # L1's degenerate candidate
        g, SJ = got[(cr.BATCH_CASES.index("L1"), (0, 0), kind)]
        assert g["status"] == "out_of_reach" and np.isnan(g["nis"]) and np.all(np.isnan(SJ))


def test_one_and_two_waves_of_the_assembling_sweep_give_the_same_bits(ref):
    same_bits(run_batch(ref, "asm1"), run_batch(ref, "asm2"))


# ---------------------------------------------------------------- 2. the marginal prior, far factors
def test_marginal_prior(oracle):
    """M12 as the DEVICE makes it (LM trials and two marginalising slides on the engine; no X0 prior): a = lo is the marginal
    prior's keyframe.  The reference is rebuilt from read_marginal and the states read after the slides"""
    eng, case, _ = device_marg_case(oracle, "M12", **FACTORINGS["split"][0])
    f, cref = reference(oracle, case)
    assert any(a == case.lo for a, _ in cref)
    got = gate_cases(eng, [case], [cref])
    np.testing.assert_array_equal(eng.get_states(0, 0, case.prob["n"]), case.states)
    check("M12", case, cref, got, 0, "device-made marginal prior")
    eng.close()


def test_far_factors(ref):
    """F17 and G17 with their far factors alive, in the LDS form of C and, with max_far_factors = 16 and far_big_forms = 1, in the
    device-memory form: the same bits, both within the bars; one candidate sits on a far factor's own pair.  L17, the third window,
    holds none.  G17 at the same states WITHOUT its far factors lies beyond the bar: the test sees the downdate"""
    names = cr.FAR_CASES + ("L17",)
    cases = [ref(n)[0]["case"] for n in names]
    crefs = [ref(n)[1] for n in names]
    cap = 17 + 8

    def run(with_far=True, **kw):
        eng = make_engine(len(cases), cap, rr.LAMBDA, **kw)
        for w, c in enumerate(cases):
            load(eng, w, c if with_far else ref("L17")[0]["case"], cap)       # (F17, G17 and L17 are one problem: seed 7, 17 keyframes)
        out = gate_cases(eng, cases, crefs)
        eng.close()
        return out

    lds, big = run(), run(max_far_factors=16, far_big_forms=1)
    for w, name in enumerate(names):
        assert name == "L17" or cl.FAR_PAIR in crefs[w]
        check(name, cases[w], crefs[w], lds, w, "the LDS form")
        check(name, cases[w], crefs[w], big, w, "max_far_factors = 16, far_big_forms = 1")
    same_bits(lds, big)
    band = run(with_far=False)
    w = names.index("G17")
    for c, r in crefs[w].items():
        e = cl.err_joint(band[(w, c, "consistent")][1], r["SJ"])
        print(f"G17 {c}: the band alone lies {e / cl.bar('G17'):.3g} x the bar from the reference")
        assert e > 10.0 * cl.bar("G17")
    same_bits({k: v for k, v in lds.items() if k[0] == 2}, {k: v for k, v in band.items() if k[0] == 2})      # L17: the band's bits


# ---------------------------------------------------------------- 3. independence
def test_a_candidate_does_not_depend_on_its_company(ref):
    """alone on a one-window engine: the bits it has inside the batch with three others on its window.  And four candidates on
    eight distinct keyframes (48 columns from the smallest keyframe on) against each of them alone (12 columns from its own a)"""
    batch = run_batch(ref, "split")
    kw = FACTORINGS["split"][0]
    for name in ("P13", "L35"):
        f, cref = ref(name)
        case, w = f["case"], cr.BATCH_CASES.index(name)
        assert len(cref) == 4
        eng = make_engine(1, BATCH_CAPACITY, rr.LAMBDA, **kw)
        load(eng, 0, case, BATCH_CAPACITY)
        for c in cref:
            for kind in cl.KINDS:
                g = eng.gate_closures([0], [c[0]], [c[1]], cref[c]["recs"][kind][None], threshold=THRESHOLD)[0]
                same_bits({0: (g, eng.read_closure_joint(0))}, {0: batch[(w, c, kind)]})
        if name == "P13":
            lo, hi = case.lo, case.hi
            four = [(lo + 1, hi - 7), (lo + 3, lo + 17), (lo + 7, hi - 2), (lo + 12, hi - 1)]
            assert len({k for c in four for k in c}) == 8
            recs = np.array([cl.record(_oracle(), case, a, b, "consistent") for a, b in four])
            together = eng.gate_closures([0] * 4, [c[0] for c in four], [c[1] for c in four], recs, threshold=THRESHOLD)
            together = [(g, eng.read_closure_joint(i)) for i, g in enumerate(together)]
            for i, c in enumerate(four):
                g = eng.gate_closures([0], [c[0]], [c[1]], recs[i][None], threshold=THRESHOLD)[0]
                assert g["status"] == "ok"
                same_bits({0: (g, eng.read_closure_joint(0))}, {0: together[i]})
        eng.close()


def _oracle():
    from oracle import oracle as o
    return o


# ---------------------------------------------------------------- 4. side effects
def _snapshot(eng, cases):
    return [(eng.get_states(w, 0, c.prob["n"]), eng.read_lm(w), eng.read_result(w, c.hi - 1), eng.read_delta(w, c.lo, c.n)) for w, c in enumerate(cases)]


def _same_snapshot(x, y):
    for (s0, lm0, r0, d0), (s1, lm1, r1, d1) in zip(x, y):
        assert np.array_equal(s0, s1) and lm0 == lm1 and np.array_equal(d0, d1)
        assert np.array_equal(r0.pop("state"), r1.pop("state")) and r0 == r1


def test_side_effects(ref):
    names = ("L9", "P3", "L17")
    cases = [ref(n)[0]["case"] for n in names]
    crefs = [ref(n)[1] for n in names]

    def engine():
        eng = make_engine(len(cases), 32, rr.LAMBDA, **FACTORINGS["split"][0])
        for w, c in enumerate(cases):
            load(eng, w, c, 32)
        eng.iterate(2)
        eng.marginals()
        return eng

    eng, twin = engine(), engine()
    assert eng.closure_gate_status()[2:] == (0, 0) and twin.closure_gate_status()[2:] == (0, 0)       # no closure buffers yet
    before = _snapshot(eng, cases)
    sig = [eng.read_marginals(w, c.lo, c.n, cross=True) for w, c in enumerate(cases)]
    got = gate_cases(eng, cases, crefs)
    assert all(g["status"] == "ok" for g, _ in got.values())
    _same_snapshot(before, _snapshot(eng, cases))                                   # states, LM state, result block, increment
    for w, c in enumerate(cases):                                                   # the marginals made before, and their validity
        cov, cross = eng.read_marginals(w, c.lo, c.n, cross=True)
        assert np.array_equal(cov, sig[w][0]) and np.array_equal(cross, sig[w][1])
    h2d, kern, scratch, results = eng.closure_gate_status()
    assert kern > 0.0 and scratch > 0 and results > 0
    eng.iterate(2)
    twin.iterate(2)
    _same_snapshot(_snapshot(eng, cases), _snapshot(twin, cases))                   # the next solve: the bits of an engine that never gated
    assert twin.closure_gate_status()[2:] == (0, 0)
    eng.close()
    twin.close()


# ---------------------------------------------------------------- 5. statuses and refusals
def refused(call, code):
    with pytest.raises(VilFusionError) as e:
        call()
    assert e.value.code == code, e.value


def test_statuses_and_refusals(ref):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    names = ("L1", "L9", "P3")
    cases = [ref(n)[0]["case"] for n in names]
    eng = make_engine(len(cases), 32, rr.LAMBDA, **FACTORINGS["split"][0])
    for w, c in enumerate(cases):
        load(eng, w, c, 32)
    refused(lambda: eng.read_closure_gate(0), -1)                                   # a read before any call
    refused(lambda: eng.read_closure_gate_all(), -1)
    p3 = cases[2]
    ok = (p3.lo, p3.hi - 1)
    rec = ref("P3")[1][ok]["recs"]["consistent"]
    cands = [(0, 0, 0), (1, -1, 5), (1, 5, 5), (1, 6, 2), (2, p3.lo - 1, p3.lo + 4), (2, p3.lo + 2, p3.hi), (2, ok[0], ok[1])]
    want = ["out_of_reach", "none", "out_of_reach", "out_of_reach", "out_of_reach", "out_of_reach", "ok"]
    recs = np.array([NO_REC] * 6 + [rec])
    got = eng.gate_closures(*map(list, zip(*cands)), recs, threshold=THRESHOLD)
    assert [g["status"] for g in got] == want
    for i, g in enumerate(got[:-1]):
        assert not g["rejected"] and np.isnan(g["nis"]) and np.isnan(g["nis_measurement"]) and np.all(np.isnan(g["xi"]))
        assert np.all(np.isnan(eng.read_closure_joint(i)))
    last = eng.read_closure_gate(6, joint=True)
    assert np.isfinite(last["nis"]) and np.all(np.isfinite(last["joint_covariance"]))
    refused(lambda: eng.read_closure_gate(7), -2)                                   # at the count
    assert eng.read_closure_gate_all()[0].size == 7
    with pytest.raises(ValueError):                                                 # (the library writes the count's entries: another n is refused in Python)
        eng.read_closure_gate_all(3)
    refused(lambda: eng.read_closure_gate(-1), -2)
    # five candidates on one window: VF_ERR_CAPACITY, the last result still readable
    refused(lambda: eng.gate_closures([2] * 5, [ok[0]] * 5, [ok[1]] * 5, np.array([rec] * 5)), -6)
    again = eng.read_closure_gate(6, joint=True)
    assert again["nis"] == last["nis"] and np.array_equal(again["joint_covariance"], last["joint_covariance"])
    refused(lambda: eng.gate_closures([3], [0], [1], rec[None]), -2)                # a window that does not exist
    refused(lambda: eng.gate_closures([-1], [0], [1], rec[None]), -2)
    assert eng.read_closure_gate(6)["nis"] == last["nis"]
    refused(lambda: _lib.check(eng._l.vf_engine_gate_closures(eng._h, -1, None, None, None, None, 0.0)), -1)
    refused(lambda: _lib.check(eng._l.vf_engine_gate_closures(eng._h, 1, None, None, None, None, 0.0)), -1)
    eng.close()
    one = make_engine(1, 128, rr.LAMBDA, **FACTORINGS["split"][0])                   # a read after compact
    load(one, 0, p3, 128)
    assert one.gate_closures([0], [ok[0]], [ok[1]], rec[None])[0]["status"] == "ok"
    one.set_range(0, 64, 64)                                                        # (nothing alive below the shift)
    assert one.read_closure_gate(0)["status"] == "ok"                               # the result is of the call that wrote it
    one.compact(64)
    refused(lambda: one.read_closure_gate(0), -1)
    one.close()
    sh = Engine(EngineOpts(windows=1, capacity=128, chunks=2))                      # a time-sharded engine
    sh.set_shard(0, 2)
    refused(lambda: sh.gate_closures([0], [0], [1], NO_REC[None]), -1)
    sh.close()


# ---------------------------------------------------------------- 5b. the estimate of a reference-compat engine
def test_from_estimate_reads_the_trial_buffer(oracle, ref):
    """VF_GATE_FROM_ESTIMATE: T_a, T_b -- xi, r, nis_measurement -- are the trial buffer's (get_estimate), where a reference-compat
    engine keeps its estimate; without the flag the current buffer's.  Sigma_J is of the current buffer's linearisation either way:
    the same bits.  One increment is solved and retracted into the trial buffer, never accepted: the two buffers differ"""
    f, cref = ref("L9")
    case = f["case"]
    eng = make_engine(1, 32, rr.LAMBDA, **FACTORINGS["split"][0])
    load(eng, 0, case, 32)
    eng.linearize(0)
    eng.assemble()
    eng.solve()
    eng.retract()
    theta, est = eng.get_states(0, 0, case.n), eng.get_estimate(0, 0, case.n)
    np.testing.assert_array_equal(theta, case.states[:case.n])
    assert np.abs(est - theta).max() > 1e-6
    (a, b), c = next((k, v) for k, v in cref.items() if k == (case.lo, case.hi - 1))
    rec = c["recs"]["consistent"]
    out = {}
    for flag in (False, True):
        g = eng.gate_closures([0], [a], [b], rec[None], threshold=THRESHOLD, from_estimate=flag)[0]
        assert g["status"] == "ok"
        out[flag] = (g, eng.read_closure_joint(0))
        x = est if flag else theta
        xi = oracle.between_factor(rec, x[a], x[b], whiten=False)[0]
        r = oracle.between_factor(rec, x[a], x[b])[0]
        print(f"from_estimate = {flag}: xi error {np.abs(g['xi'] - xi).max():.1e}, nis_measurement {g['nis_measurement']:.6e} (oracle {float(r @ r):.6e})")
        assert np.abs(g["xi"] - xi).max() <= 1e-12 and abs(g["nis_measurement"] - float(r @ r)) <= 1e-9 * float(r @ r)
    np.testing.assert_array_equal(out[False][1], out[True][1])
    assert np.abs(out[False][0]["xi"] - out[True][0]["xi"]).max() > 1e-7
    np.testing.assert_array_equal(eng.get_estimate(0, 0, case.n), est)
    eng.close()


def test_reference_compat_handle_gates_from_the_estimate(oracle):
    """a reference_compat handle keeps theta in the current buffer and the estimate beside it: vf_gate_closure's innovation is that
    of the ESTIMATE (vf_get_trajectory), as vf_gate_between's newer end is"""
    from vil_sensor_fusion_amd import synth
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 24
    seq = synth.make_sequence(seed=12, n_kf=n)
    gm = GraphManager(capacity=128, lag=0, reference_compat=True)
    gm.setInitialState(seq.gt_states[0])
    _feed(gm, seq, 1, n, _imu_stream(seq))
    est = gm.trajectory(0, n)
    a, b = 3, n - 1
    q, t = _true_closure(seq, a, b)
    g = gm.gate_closure(a, b, (q, t), cl.COV36, threshold=THRESHOLD)
    rec = np.zeros(28)
    rec[0:4], rec[4:7], rec[7:28] = q, t, oracle.sqrt_info_upper(cl.COV36)
    xi = oracle.between_factor(rec, est[a], est[b], whiten=False)[0]
    r = oracle.between_factor(rec, est[a], est[b])[0]
    print(f"reference_compat handle ({a}, {b}): {g['status']}, nis {g['nis']:.4f}, xi error against the estimate {np.abs(g['xi'] - xi).max():.1e}")
    assert g["status"] == "ok" and np.isfinite(g["nis"]) and g["nis"] <= g["nis_measurement"]
    assert np.abs(g["xi"] - xi).max() <= 1e-12 and abs(g["nis_measurement"] - float(r @ r)) <= 1e-9 * max(float(r @ r), 1e-3)
    gm.close()


# ---------------------------------------------------------------- 6. the handle
def _feed(gm, seq, k0, k1, imu):
    """keys k0 .. k1 - 1 of the sequence into the handle, a solve per key (tests/test_gpu_marginals_far.py::_feed)"""
    traj_t, acc, gyr, at = imu
    for k in range(k0, k1):
        while at[0] < traj_t.size and traj_t[at[0]] <= seq.kf_time[k] + 0.01:
            gm.addIMUMeasurement(traj_t[at[0]], acc[at[0]], gyr[at[0]])
            at[0] += 1
        gm.reserveNode(seq.kf_time[k])
        for a, b, q, t, c in zip(seq.btw_a, seq.btw_b, seq.btw_q, seq.btw_t, seq.btw_cov):
            if b == k and a >= 1:
                gm.addBetweenFactor(int(a), int(b), (q, t), np.eye(6) * c)
        gm.solve()


def _imu_stream(seq):
    from vil_sensor_fusion_amd import synth
    traj_t = synth.IMU_PHASE + np.arange(0, int((seq.kf_time[-1] + 0.5) * synth.IMU_RATE)) / synth.IMU_RATE
    traj = synth.Trajectory(seq.seed, seq.kf_time[-1] + 1.0)
    rng = np.random.default_rng([seq.seed, 0xBEEF])
    acc = traj.specific_force(traj_t) + rng.normal(size=(traj_t.size, 3)) * synth.IMU_NOISE
    gyr = traj.body_rate(traj_t) + rng.normal(size=(traj_t.size, 3)) * synth.IMU_NOISE
    return traj_t, acc, gyr, [0]


def _true_closure(seq, a, b, d=None):
    """(q, t) of T_a^-1 T_b of the ground truth, moved by the tangent vector d"""
    from vil_sensor_fusion_amd import synth
    o = _oracle()
    Ra, Rb = synth.quat_to_rot(seq.gt_states[a, :4]), synth.quat_to_rot(seq.gt_states[b, :4])
    R, t = Ra.T @ Rb, Ra.T @ (seq.gt_states[b, 4:7] - seq.gt_states[a, 4:7])
    if d is not None:
        Rd, td = o.se3_exp(np.asarray(d, dtype=np.float64))
        R, t = R @ Rd, t + R @ td
    return synth.rot_to_quat(R), t


def test_handle(oracle):
    from tests.test_gpu_marginals import EPS, dense_inverse
    from tests.test_gpu_marginals_far import _dense_from_oracle
    from vil_sensor_fusion_amd import synth
    from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS
    from vil_sensor_fusion_amd.graph_manager import GraphManager
    n = 40
    seq = synth.make_sequence(seed=12, n_kf=n)
    imu = _imu_stream(seq)
    gm = GraphManager(capacity=128, iterations=4, lag=0)
    gm.setInitialState(seq.gt_states[0])         # (the synthetic vehicle is already moving at t = 0)
    _feed(gm, seq, 1, n - 4, imu)
    new, early = n - 5, 3
    cov = cl.COV36
    staged = (gm.graphSize(), gm.imuQueueSize())
    g = gm.gate_closure(early, new, _true_closure(seq, early, new), cov, threshold=THRESHOLD)
    print(f"true closure ({early}, {new}): {g['status']}, nis {g['nis']:.3f} (measurement alone {g['nis_measurement']:.3f})")
    assert g["status"] == "ok" and g["nis"] < THRESHOLD and not g["rejected"] and g["nis"] <= g["nis_measurement"]
    assert np.array_equal(g["joint_covariance"], g["joint_covariance"].T) and np.all(np.linalg.eigvalsh(g["joint_covariance"]) > 0)
    assert (gm.graphSize(), gm.imuQueueSize()) == staged
    bad = gm.gate_closure(early, new, _true_closure(seq, early, new, [0.0, 0.0, 0.0, 3.0, -2.0, 1.0]), cov, threshold=THRESHOLD)
    print(f"the same closure displaced by metres: {bad['status']}, nis {bad['nis']:.3e}")
    assert bad["status"] == "ok" and bad["rejected"] and bad["nis"] > THRESHOLD
    assert (gm.graphSize(), gm.imuQueueSize()) == staged
    # the true closure is added and becomes a far factor; a second closure is gated with the first alive
    gm.addBetweenFactor(early, new, _true_closure(seq, early, new), cov)
    _feed(gm, seq, n - 4, n, imu)
    assert len(gm.far_weights()) == 1                                               # it is a far factor, and alive
    a2, b2 = 8, n - 1
    q2, t2 = _true_closure(seq, a2, b2)
    g2 = gm.gate_closure(a2, b2, (q2, t2), cov, threshold=THRESHOLD)
    assert g2["status"] == "ok" and np.isfinite(g2["nis"])
    st = gm.trajectory(0, n)
    imu_rec = np.stack([gm.imuFactor(k) for k in range(1, n)])
    gm.close()
    # nothing was staged or consumed: a handle fed the same stream that never gated has the same bits
    twin = GraphManager(capacity=128, iterations=4, lag=0)
    twin.setInitialState(seq.gt_states[0])
    imu_t = _imu_stream(seq)
    _feed(twin, seq, 1, n - 4, imu_t)
    twin.addBetweenFactor(early, new, _true_closure(seq, early, new), cov)
    _feed(twin, seq, n - 4, n, imu_t)
    assert np.array_equal(twin.trajectory(0, n), st)
    twin.close()
    # numpy on the oracle's dense H of the same graph (the closure's rows in it) at the handle's states
    m = seq.btw_a >= 1
    far_rec = np.zeros(28)
    far_rec[0:4], far_rec[4:7], far_rec[7:28] = *_true_closure(seq, early, new), oracle.sqrt_info_upper(cov)
    prob = dict(n=n, states=st, imu=np.vstack([np.zeros((1, imu_rec.shape[1])), imu_rec]),
                btw_a=np.concatenate([seq.btw_a[m], [early]]).astype(np.int32), btw_b=np.concatenate([seq.btw_b[m], [new]]).astype(np.int32),
                btw=np.vstack([synth.between_records(seq)[m], far_rec]), prior=synth.prior_record(seq.gt_states[0], REFERENCE_PRIOR_SIGMAS),
                gravity=np.array([0.0, 0.0, -9.81]))
    Sref, cs, _ = dense_inverse(_dense_from_oracle(oracle, prob))
    SJ = cl.joint(Sref, a2, b2)
    e = cl.err_joint(g2["joint_covariance"], SJ)
    rec2 = np.zeros(28)
    rec2[0:4], rec2[4:7], rec2[7:28] = q2, t2, oracle.sqrt_info_upper(cov)
    res, Ja, Jb = oracle.between_factor(rec2, st[a2], st[b2])
    J = np.hstack([Ja, Jb])
    y = np.linalg.solve(np.eye(6) + J @ SJ @ J.T, res)
    nis = float(res @ y)
    # to first order d nis = -y^T J dSigma J^T y: |y|^T |J| E |J|^T |y| with E_pq = cond eps sqrt(Sigma_pp Sigma_qq), the bar
    # tests/test_gpu_marginals_far.py holds these blocks to, plus NIS_BAR x nis for the gate's own arithmetic
    d = np.sqrt(np.diag(SJ))
    u = np.abs(J).T @ np.abs(y)
    bound = float(u @ (cs * EPS * np.outer(d, d)) @ u) + cl.NIS_BAR * nis
    print(f"second closure ({a2}, {b2}) with the first alive: nis {g2['nis']:.9e}, numpy on the oracle's dense H {nis:.9e}, |difference| "
          f"{abs(g2['nis'] - nis):.3e} (bound {bound:.3e}); Sigma_J error {e:.3e} (bar cond eps = {cs * EPS:.3e})")
    assert e < cs * EPS and abs(g2["nis"] - nis) <= bound
    # a lag-limited handle: a key that has left the window is out of reach, one inside is tested
    lag = GraphManager(capacity=128, iterations=3, lag=12)
    lag.setInitialState(seq.gt_states[0])
    imu = _imu_stream(seq)
    _feed(lag, seq, 1, 30, imu)
    out = lag.gate_closure(early, 29, _true_closure(seq, early, 29), cov, threshold=THRESHOLD)
    assert out["status"] == "out_of_reach" and np.isnan(out["nis"]) and not out["rejected"]
    assert lag.gate_closure(22, 29, _true_closure(seq, 22, 29), cov, threshold=THRESHOLD)["status"] == "ok"
    lag.close()
