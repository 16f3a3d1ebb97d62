"""-m gpu: robust losses on band between factors (vf_engine_set_between_loss; include/vilfusion.h "Robust loss on band between
factors") against tests/robust_ref.py, whose cases tests/test_robust_ref_host.py holds to their conditions on the CPU.

Shapes: 3 windows (windows 1 and 2 are asserted like window 0), capacity 128 with the keyframes at slots 59 .. so that the range
crosses the AoSoA tile boundary at 64, bandwidth 3 with between factors at distances 1, 2 and 3, robust and Gaussian factors mixed
in every window, residual norms inside, at and far outside k for each loss, a factor with r = 0 exactly and one at 1e6 k.

Bars are 16 S, S the largest error of three correct float64 evaluations against 100 digits (robust_ref); every test prints its
figures before it asserts."""
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_sharded.py)

from tests import robust_ref as R

pytestmark = pytest.mark.gpu
B, CAP, S0 = R.B, R.CAPACITY, R.SLOT0


def make_engine(windows=B, capacity=CAP, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    return Engine(EngineOpts(windows=windows, capacity=capacity, **kw))


def load(eng, w, prob, states, s0=S0):
    n = prob["n"]
    eng.set_states(w, s0, states)
    eng.set_imu(w, s0 + 1, prob["imu"][1:])
    eng.set_between(w, prob["btw_a"] + s0, prob["btw_b"] + s0, prob["btw"])
    eng.set_prior(w, s0, prob["prior"])
    eng.set_range(w, s0, s0 + n)


def set_losses(eng, w, case, s0=S0):
    eng.set_between_loss(w, case["prob"]["btw_b"] + s0, list(case["loss"]), case["k"])


def make_arrays(eng):
    """the engine's loss arrays, with no factor's loss changed: a loss on slot 0, which holds no factor, is inert"""
    eng.set_between_loss(0, [0], "huber", 1.0)


def snapshot(eng, n, s0=S0):
    return [(eng.get_states(w, s0, n), eng.read_lm(w)) for w in range(eng.windows)]


def same_snapshots(a, b):
    for (xa, la), (xb, lb) in zip(a, b):
        np.testing.assert_array_equal(xa, xb)
        assert la == lb, (la, lb)


# ---------------------------------------------------------------- 5. linearisation
@pytest.fixture(scope="module")
def lin_run():
    """twin (no losses) and robust engine on the same records and states; both buffers linearised: {which: (twin, robust)} read-backs"""
    cases = R.lin_cases()
    twin, rob = make_engine(), make_engine()
    for eng in (twin, rob):
        for w, c in enumerate(cases):
            load(eng, w, c["prob"], c["states"])
    make_arrays(rob)
    # a trial buffer that differs from the current one: one solve and retraction, with no loss set yet (the arrays exist and hold
    # none: the same increments to the bit, asserted -- test_nothing_changes_when_nothing_is_asked holds that on its own)
    for eng in (twin, rob):
        eng.linearize(0)
        eng.decide(True)
        eng.assemble()
        eng.solve()
    for w in range(B):
        np.testing.assert_array_equal(twin.read_delta(w, S0, R.LIN_N), rob.read_delta(w, S0, R.LIN_N))
        assert np.max(np.abs(twin.read_delta(w, S0, R.LIN_N))) > 1e-6
    for eng in (twin, rob):
        eng.retract()
    for w, c in enumerate(cases):
        set_losses(rob, w, c)
    out = {}
    for which in (0, 1):
        twin.linearize(which)
        rob.linearize(which)
        out[which] = [(twin.read_between_lin(w, S0, R.LIN_N, which), rob.read_between_lin(w, S0, R.LIN_N, which)) for w in range(B)]
    got = [rob.get_between_loss(w, S0, R.LIN_N) for w in range(B)]
    twin.close()
    rob.close()
    return cases, out, got


def _factor_figures(cases, run, which):
    """per (window, factor): (loss, ratio, S, error, bits equal) from the twin's doubles"""
    rows = []
    for w, c in enumerate(cases):
        (r, Ja, Jb), (rh, Jah, Jbh) = run[which][w]
        for f, b in enumerate(c["prob"]["btw_b"]):
            loss, k = int(c["loss"][f]), float(c["k"][f])
            J, Jh = np.hstack([Ja[b], Jb[b]]), np.hstack([Jah[b], Jbh[b]])
            want = R.mp_hat(r[b], J, loss, k)
            rows.append(dict(w=w, f=f, loss=loss, ratio=c["ratio"][f], S=R.hat_S(r[b], J, loss, k), err=R.hat_error(rh[b], Jh, r[b], J, loss, k, want),
                             same=bool(np.array_equal(r[b], rh[b]) and np.array_equal(J, Jh)), s=float(np.linalg.norm(r[b])), k=k,
                             identity=want[2] == 1 and want[3] == 0))
    return rows


def _own_S(S, x):
    """the S a factor is held to: the common one, or for a Huber factor within rounding distance of its threshold its own -- which
    must itself be what rounding explains (robust_ref.near_threshold_cap), so that nothing hides behind it"""
    if not R.near_threshold(x["loss"], x["ratio"]):
        return S
    assert x["S"] <= R.near_threshold_cap(x["ratio"]), x
    return max(S, x["S"])


@pytest.mark.parametrize("which", [0, 1])
def test_linearisation_matches_the_square_root_form(lin_run, which):
    """r^ and J^ of every factor against the 100-digit evaluation from the twin's r and J, within 16 S entry-wise (normalised by
    |alpha| |J_ij| + |gamma| |r_i| sum_l |r_l J_lj|); S = the largest error of the three float64 evaluations over the factors of
    all windows -- except a Huber factor within 2^-30 of its threshold, whose gamma ~ s - k no float64 norm resolves: its S is its own,
    and capped by what the rounding of the norm explains (_own_S)."""
    cases, run, _ = lin_run
    rows = _factor_figures(cases, run, which)
    S = max(x["S"] for x in rows if not R.near_threshold(x["loss"], x["ratio"]))
    assert 0.0 < S < 64 * R.EPS, S
    for x in rows:
        bar = 16 * _own_S(S, x)
        print(f"which {which} window {x['w']} factor {x['f']}: {R.NAMES[x['loss']]:14s} s/k {x['ratio']} s {x['s']:.3e}: error {x['err']:.3e} = {x['err'] / bar:.3f} of the bar {bar:.2e}"
              f"{' (same bits as the twin)' if x['same'] else ''}")
    for x in rows:
        bar = 16 * _own_S(S, x)
        assert x["err"] <= bar, x
        if x["identity"] and not (R.near_threshold(x["loss"], x["ratio"]) and x["ratio"] > 1):
            assert x["same"], x           # a slot without a loss, a Huber inlier: the twin's bits
    if which == 1:
        return      # (s / k is what the case was built for at the loaded states; the trial buffer's states have moved on)
    # the figures are of what they claim: outliers at 1e6 k, an exact zero, inliers, and robust factors that changed
    assert any(x["s"] == 0.0 and x["loss"] != R.NONE for x in rows) and any(x["ratio"] == 1e6 for x in rows)
    assert all(not x["same"] for x in rows if x["loss"] != R.NONE and x["ratio"] is not None and x["ratio"] >= 3.0)
    assert {x["w"] for x in rows if not x["same"]} == {0, 1, 2}


def test_trial_buffer_differs_from_the_current_one(lin_run):
    _, run, got = lin_run
    for w in range(B):
        assert not np.array_equal(run[0][w][0][0], run[1][w][0][0])
    cases = lin_run[0]
    for w, c in enumerate(cases):         # ... and the attributes read back as they were set
        b = c["prob"]["btw_b"]
        np.testing.assert_array_equal(got[w][0][b], c["loss"])
        np.testing.assert_array_equal(got[w][1][b], np.where(c["loss"] == R.NONE, 0.0, c["k"]))


# ---------------------------------------------------------------- 10. factor errors
def test_factor_errors_are_rho(lin_run):
    """vf_engine_factor_errors gives rho(s) for a robust factor.  Bar: r^ is within b = 16 S entry-wise (the linearisation test), so
    0.5 sum r^_i^2 is within 2 b + b^2 of rho, plus 4 eps for its six products, five additions and the halving."""
    from vil_sensor_fusion_amd import robust
    cases, run, _ = lin_run
    rows = _factor_figures(cases, run, 0)
    S = max(x["S"] for x in rows if not R.near_threshold(x["loss"], x["ratio"]))
    eng = make_engine()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["states"])
        set_losses(eng, w, c)
    eng.factor_errors(relinearize=True)
    checked = 0
    for w, c in enumerate(cases):
        _, eb, a = eng.read_factor_errors(w, S0, R.LIN_N)
        r = run[0][w][0][0]
        for f, b in enumerate(c["prob"]["btw_b"]):
            loss, k = int(c["loss"][f]), float(c["k"][f])
            with R.mp.workdps(R.DPS):
                s = R.mp.sqrt(sum(R.mp.mpf(float(x)) ** 2 for x in r[b]))
                rho = R.mp_rho(loss, k, s)
                e = float(abs(R.mp.mpf(float(eb[b])) - rho) / rho) if rho != 0 else (0.0 if eb[b] == 0.0 else math.inf)
                wt = float(R.mp_drho(loss, k, s) / s) if s != 0 else 1.0
            x = [y for y in rows if y["w"] == w and y["f"] == f][0]
            b16 = 16 * _own_S(S, x)
            bar = 2 * b16 + b16 * b16 + 4 * R.EPS
            print(f"window {w} factor {f}: {R.NAMES[loss]:14s} error {eb[b]:.6e}, off by {e:.3e} = {e / bar:.3f} of the bar {bar:.2e}")
            assert a[b] == c["prob"]["btw_a"][f] + S0
            assert e <= bar, (w, f)
            # the weight from the error alone, where the error determines it: |d ln w / d ln e| (R.weight_condition) amplifies the error's own
            cond = R.weight_condition(loss, k, float(s))
            if loss != R.NONE and cond < 1e3:
                got = robust.weight_from_error(loss, k, float(eb[b]))
                assert abs(got - wt) <= ((1 + cond) * bar + 8 * R.EPS) * wt, (w, f, got, wt)
                checked += 1
    assert checked >= 12
    eng.close()


# ---------------------------------------------------------------- 6. optimum
def run_opt(loss, form=None, **kw):
    cases = R.opt_cases(loss)
    eng = make_engine(**kw)
    if form is not None:
        assert eng.solve_form() == form, eng.solve_form()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["start"])
        set_losses(eng, w, c)
    eng.iterate(R.OPT_TRIALS)
    out = snapshot(eng, R.OPT_N)
    eng.close()
    return cases, out


def check_opt(oracle, loss, cases, out, what=""):
    S = max(R.optima(loss, w)["S"] for w in range(B))
    assert S < 1e-6, S                 # (BASELINE's bar on positions: above it the case would be ill-posed)
    bar = 16 * S
    figures = []
    for w, c in enumerate(cases):
        x, lm = out[w]
        o = R.optima(loss, w)
        e = R.position_error(x, o["irls"])
        ad = R.addends(oracle, c["prob"], x, c["loss"], c["k"])
        host = math.fsum(ad)
        cbar = (ad.size + 8) * R.EPS * math.fsum(np.abs(ad))
        figures.append((e, abs(lm["cost"] - host), cbar, lm))
        print(f"{R.NAMES[loss]} {what} window {w}: position error {e:.3e} = {e / bar:.3g} of the bar {bar:.2e} (S {S:.2e}; the Gaussian optimum is "
              f"{R.position_error(o['gauss'], o['irls']):.2e} away); cost {lm['cost']:.17g}, host {host:.17g}, off by {abs(lm['cost'] - host):.2e} = "
              f"{abs(lm['cost'] - host) / cbar:.3g} of the bar {cbar:.2e}; {lm['accepted']} accepted, {lm['rejected']} rejected, {lm['solve_failures']} failed")
    for e, dc, cbar, lm in figures:
        assert lm["solve_failures"] == 0
        assert e <= bar, (e, bar)
        assert dc <= cbar, (dc, cbar)


@pytest.mark.parametrize("loss", R.LOSSES)
def test_optimum(oracle, loss):
    """LM at the default tuning, termination rule off, OPT_TRIALS trials, against the dense host IRLS optimum (GTSAM's form, not the
    kernel's); the cost of vf_engine_read_lm against the host's sum of rho at the returned states.

    Measured on an MI355X: position errors between 1e-17 and 4e-13 m against bars of 8.5e-13 (Huber), 1.4e-11 (Cauchy) and 5.8e-12 m
    (Geman-McClure), the Gaussian optimum 1.3e-5 to 3e-5 m away; the cost off by at most 1.1e-14 against bars of 7e-14 to 1e-12."""
    cases, out = run_opt(loss)
    check_opt(oracle, loss, cases, out)


# ---------------------------------------------------------------- 7. every solve form
FORMS = {       # vf_engine_solve_form's name, and the switches that reach it as tests/test_gpu_direct_small.py reaches it
    "one_wave": ("one_wave", dict(chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, solve_split_min=0)),
    "one_wave_split": ("one_wave_split", dict(chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, solve_split_min=1)),
    "assembling_1": ("assembling", dict(chunks=1, sweep_two_sided_max=0, solve_split_min=0, solve_assemble_min=1, solve_assemble_waves=1)),
    "assembling_2": ("assembling", dict(chunks=1, sweep_two_sided_max=0, solve_split_min=0, solve_assemble_min=1, solve_assemble_waves=2)),
    "two_sided": ("two_sided", dict(chunks=1, sweep_two_sided_max=1 << 20)),
    "partitioned": ("partitioned", dict(chunks=2)),
    "refined": (None, dict(refine_iterations=2)),
    "gtsam_accept_rule": (None, dict(min_model_fidelity=1e-3)),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_solve_form_consumes_it(oracle, form):
    name, kw = FORMS[form]
    cases, out = run_opt(R.HUBER, form=name, **kw)
    check_opt(oracle, R.HUBER, cases, out, form)


# ---------------------------------------------------------------- 8. nothing changes when nothing is asked
def _three_trials(prepare):
    cases = R.opt_cases(R.HUBER)
    eng = make_engine()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["start"])
    prepare(eng, cases)
    eng.iterate(3)
    out = snapshot(eng, R.OPT_N)
    eng.close()
    return out


def test_nothing_changes_when_nothing_is_asked():
    plain = _three_trials(lambda eng, cases: None)
    # (a) the arrays exist and hold no loss on any factor
    same_snapshots(plain, _three_trials(lambda eng, cases: make_arrays(eng)))

    # (b) Huber with a threshold nothing reaches
    def huge(eng, cases):
        for w, c in enumerate(cases):
            eng.set_between_loss(w, c["prob"]["btw_b"] + S0, "huber", 1e30)
    same_snapshots(plain, _three_trials(huge))

    # (c) two runs of the same robust engine -- which is not the Gaussian one
    def robust(eng, cases):
        for w, c in enumerate(cases):
            set_losses(eng, w, c)
    a, b = _three_trials(robust), _three_trials(robust)
    same_snapshots(a, b)
    for w in range(B):
        assert not np.array_equal(a[w][0], plain[w][0])


# ---------------------------------------------------------------- 9. slot semantics
def test_slot_semantics():
    from vil_sensor_fusion_amd import synth
    cases = R.opt_cases(R.HUBER)
    n = R.OPT_N
    eng = make_engine()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["start"], s0=64)
    li, lk = eng.get_between_loss(1, 0, CAP)
    assert not li.any() and not lk.any()                       # no arrays: none everywhere
    slots = np.arange(64, 64 + n + 2, dtype=np.int32)          # (the two behind the window's end hold no factor: inert)
    ids = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1], dtype=np.int32)
    ks = 0.5 + np.arange(slots.size)
    for w in range(B):
        eng.set_between_loss(w, slots, list(ids), ks + w)
    for w in range(B):
        li, lk = eng.get_between_loss(w, 0, CAP)
        np.testing.assert_array_equal(li[64:64 + slots.size], ids)
        np.testing.assert_array_equal(lk[64:64 + slots.size], ks + w)
        assert not li[:64].any() and not li[64 + slots.size:].any()
    # vf_engine_set_between resets the slot it writes, and only that one (window 1)
    p = cases[1]["prob"]
    f = 2
    eng.set_between(1, p["btw_a"][f:f + 1] + 64, p["btw_b"][f:f + 1] + 64, p["btw"][f:f + 1])
    want = ids.copy()
    want[p["btw_b"][f]] = 0
    li, lk = eng.get_between_loss(1, 64, slots.size)
    np.testing.assert_array_equal(li, want)
    assert lk[p["btw_b"][f]] == 0.0
    np.testing.assert_array_equal(eng.get_between_loss(0, 64, slots.size)[0], ids)
    # vf_engine_clear_between (window 2, two slots)
    eng.clear_between(2, 66, 2)
    want2 = ids.copy()
    want2[2:4] = 0
    np.testing.assert_array_equal(eng.get_between_loss(2, 64, slots.size)[0], want2)
    # vf_engine_ingest_tail writes the slot behind every window's end (64 + n): reset there, the neighbours as they were
    seq = synth.make_sequence(seed=5, n_kf=4)
    st = seq.imu_steps[seq.imu_off[1]:seq.imu_off[2]]
    off = np.arange(B + 1, dtype=np.int32) * st.shape[0]
    rec = np.tile(p["btw"][0], (B, 1))
    eng.ingest_tail(off, np.tile(st, (B, 1)), synth.CARLA_IMU_COV, np.full(B, 64 + n - 1, dtype=np.int32), rec)
    eng.ingest_status()
    for w, base in enumerate((ids, want, want2)):
        exp = base.copy()
        exp[n] = 0
        li, lk = eng.get_between_loss(w, 64, slots.size)
        np.testing.assert_array_equal(li, exp)
        assert lk[n] == 0.0 and lk[n + 1] == ks[n + 1] + w and lk[n - 1] == (ks[n - 1] + w if exp[n - 1] else 0.0)
    # vf_engine_compact(64) moves the attributes with their slots; vf_engine_grow carries them
    eng.compact(64)
    li, lk = eng.get_between_loss(1, 0, CAP)
    exp = want.copy()
    exp[n] = 0
    np.testing.assert_array_equal(li[:slots.size], exp)
    assert not li[slots.size:].any() and lk[1] == ks[1] + 1
    eng.grow(200)
    li2, lk2 = eng.get_between_loss(1, 0, 256)
    np.testing.assert_array_equal(li2[:CAP], li)
    np.testing.assert_array_equal(lk2[:CAP], lk)
    assert not li2[CAP:].any()
    np.testing.assert_array_equal(eng.get_between_loss(2, 0, 8)[0], np.concatenate([want2[:n], [0]])[:8])
    # refusals touch nothing
    import ctypes as C
    for slot, loss, k, code in ((256, 1, 1.0, -2), (-1, 1, 1.0, -2), (3, 4, 1.0, -1), (3, -1, 1.0, -1), (3, 1, 0.0, -1), (3, 2, -1.0, -1), (3, 2, math.inf, -1), (3, 3, math.nan, -1)):
        rc = eng._l.vf_engine_set_between_loss(eng._h, 1, 1, C.byref(C.c_int32(slot)), C.byref(C.c_int32(loss)), C.byref(C.c_double(k)))
        assert rc == code, (slot, loss, k, rc)
    assert eng._l.vf_engine_set_between_loss(eng._h, B, 1, C.byref(C.c_int32(3)), C.byref(C.c_int32(1)), C.byref(C.c_double(1.0))) == -1
    np.testing.assert_array_equal(eng.get_between_loss(1, 0, 256)[0], li2)
    eng.close()


def test_asynchronous_staging_gives_the_same_attributes():
    """a one-window engine that stages asynchronously takes up to four attributes as kernel arguments: the same arrays as the
    synchronous path, and vf_engine_set_between resets there too"""
    c = R.opt_cases(R.HUBER)[0]
    p = c["prob"]
    got = []
    for asynchronous in (False, True):
        eng = make_engine(windows=1)
        load(eng, 0, p, c["start"])
        if asynchronous:
            eng.set_async(True)
        b = p["btw_b"][:4] + S0
        eng.set_between_loss(0, b, [1, 2, 3, 0], [1.5, 2.5, 3.5, 9.0])
        eng.set_between_loss(0, b[3:4] + 1, "cauchy", 0.25)
        eng.set_between(0, p["btw_a"][1:2] + S0, p["btw_b"][1:2] + S0, p["btw"][1:2])
        got.append(eng.get_between_loss(0, 0, CAP))
        eng.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])
    b = p["btw_b"][:4] + S0
    assert list(got[1][0][b]) == [1, 0, 3, 0] and got[1][0][b[3] + 1] == 2 and list(got[1][1][b]) == [1.5, 0.0, 3.5, 0.0]
