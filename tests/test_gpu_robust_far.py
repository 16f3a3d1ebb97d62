"""-m gpu: robust losses on FAR between factors (loop closures; vf_engine_set_extra_between_robust, include/vilfusion.h "Robust loss
on far between factors") against tests/robust_far_ref.py, whose cases tests/test_robust_far_ref_host.py holds to their conditions
on the CPU.

Shapes: capacity 128 with the keyframes from slot 59, so that the range crosses the AoSoA tile boundary at 64; windows of 12
keyframes, three windows per engine (windows 1 and 2 are asserted like window 0); far lists of 3 entries (the LDS forms) and of 9
on engines made with max_far_factors = 16 (more than VF_MAX_EXTRA: the device-memory forms); pairs wider than the band and a second
factor on an end key; lossy and Gaussian entries mixed in every list, every lossy entry with a k of its own.

Bars are 16 S (robust_ref for the linearisation, robust_far_ref.S_all for the optimum); every test prints its figures before it
asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before libvilfusion is loaded, as in tests/test_gpu_sharded.py)

from tests import robust_far_ref as F
from tests import robust_ref as R

pytestmark = pytest.mark.gpu
B, CAP, S0, N = F.B, F.CAPACITY, F.SLOT0, F.N


def make_engine(windows=B, capacity=CAP, **kw):
    from vil_sensor_fusion_amd import Engine, EngineOpts
    return Engine(EngineOpts(windows=windows, capacity=capacity, **kw))


def load(eng, w, prob, states, s0=S0, n=None):
    n = prob["n"] if n is None else n
    eng.set_states(w, s0, states)
    eng.set_imu(w, s0 + 1, prob["imu"][1:])
    eng.set_between(w, prob["btw_a"] + s0, prob["btw_b"] + s0, prob["btw"])
    eng.set_prior(w, s0, prob["prior"])
    eng.set_range(w, s0, s0 + n)


def set_far(eng, w, case, loss=None, k=None, s0=S0):
    a, b, rec = case["far"]
    if loss is None:
        eng.set_extra_between(w, a + s0, b + s0, rec)
    else:
        eng.set_extra_between(w, a + s0, b + s0, rec, loss=list(loss), k=k)


def snapshot(eng, n=N, s0=S0):
    return [(eng.get_states(w, s0, n), eng.read_lm(w)) for w in range(eng.windows)]


def same_snapshots(a, b):
    assert len(a) == len(b)
    for (xa, la), (xb, lb) in zip(a, b):
        np.testing.assert_array_equal(xa, xb)
        assert la == lb, (la, lb)


def differ(a, b):
    return all(not np.array_equal(xa, xb) for (xa, _), (xb, _) in zip(a, b))


# ---------------------------------------------------------------- 1. linearisation, 2. errors
@pytest.fixture(scope="module")
def lin_run():
    """twin (no losses) and robust engine on the same records and states, nine far entries per window (device-memory forms); both
    buffers linearised: {which: [(twin, robust) read-backs per window]}"""
    cases = F.lin_cases()
    twin, rob = make_engine(max_far_factors=16), make_engine(max_far_factors=16)
    for eng in (twin, rob):
        for w, c in enumerate(cases):
            load(eng, w, c["prob"], c["states"])
            set_far(eng, w, c)
    # a trial buffer that differs from the current one: one solve and retraction, no loss set yet
    for eng in (twin, rob):
        eng.linearize(0)
        eng.decide(True)
        eng.assemble()
        eng.solve()
    for w in range(B):
        np.testing.assert_array_equal(twin.read_delta(w, S0, N), rob.read_delta(w, S0, N))
        assert np.max(np.abs(twin.read_delta(w, S0, N))) > 1e-6
    for eng in (twin, rob):
        eng.retract()
    before = rob.get_extra_between_loss(0)
    for w, c in enumerate(cases):
        set_far(rob, w, c, c["loss"], c["k"])
    out = {}
    for which in (0, 1):
        twin.linearize(which)
        rob.linearize(which)
        out[which] = [(twin.read_extra_lin(w, which), rob.read_extra_lin(w, which)) for w in range(B)]
    got = [rob.get_extra_between_loss(w) for w in range(B)]
    rob.factor_errors(relinearize=True)
    errs = [rob.read_far_errors(w) for w in range(B)]
    twin.close()
    rob.close()
    return cases, out, got, before, errs


def _figures(cases, run, which):
    rows = []
    for w, c in enumerate(cases):
        (r, Ja, Jb), (rh, Jah, Jbh) = run[which][w]
        for f in range(c["loss"].size):
            loss, k = int(c["loss"][f]), float(c["k"][f])
            J, Jh = np.hstack([Ja[f], Jb[f]]), np.hstack([Jah[f], Jbh[f]])
            want = R.mp_hat(r[f], J, loss, k)
            rows.append(dict(w=w, f=f, loss=loss, ratio=c["ratio"][f], S=R.hat_S(r[f], J, loss, k), err=R.hat_error(rh[f], Jh, r[f], J, loss, k, want),
                             same=bool(np.array_equal(r[f], rh[f]) and np.array_equal(J, Jh)), s=float(np.linalg.norm(r[f])), k=k,
                             identity=want[2] == 1 and want[3] == 0, nonzero=bool(np.any(J))))
    return rows


def _own_S(S, x):
    """as tests/test_gpu_robust.py: a Huber entry within rounding distance of its threshold is held to its own S, capped"""
    if not R.near_threshold(x["loss"], x["ratio"]):
        return S
    assert x["S"] <= R.near_threshold_cap(x["ratio"]), x
    return max(S, x["S"])


@pytest.mark.parametrize("which", [0, 1])
def test_linearisation_matches_the_square_root_form(lin_run, which):
    """r^ and J^ of every far entry, through vf_engine_read_extra_lin, against the 100-digit evaluation from the lossless twin's r and
    J, within 16 S entry-wise (robust_ref's S and its near-threshold rule); entries without a loss and Huber inliers: the twin's bits"""
    cases, run, _, _, _ = lin_run
    rows = _figures(cases, run, which)
    S = max(x["S"] for x in rows if not R.near_threshold(x["loss"], x["ratio"]))
    assert 0.0 < S < 64 * R.EPS, S
    for x in rows:
        bar = 16 * _own_S(S, x)
        print(f"which {which} window {x['w']} entry {x['f']}: {R.NAMES[x['loss']]:14s} s/k {x['ratio']} s {x['s']:.3e}: error {x['err']:.3e} = {x['err'] / bar:.3f} of the bar {bar:.2e}"
              f"{' (same bits as the twin)' if x['same'] else ''}")
    for x in rows:
        assert x["nonzero"], x                     # (the twin did linearise the entry)
        assert x["err"] <= 16 * _own_S(S, x), x
        if x["identity"] and not (R.near_threshold(x["loss"], x["ratio"]) and x["ratio"] > 1):
            assert x["same"], x
    if which == 1:
        return
    assert any(x["s"] == 0.0 and x["loss"] != R.NONE for x in rows) and any(x["ratio"] == 1e6 for x in rows)
    assert all(not x["same"] for x in rows if x["loss"] != R.NONE and x["ratio"] is not None and x["ratio"] >= 3.0)
    assert {x["w"] for x in rows if not x["same"]} == {0, 1, 2}


def test_buffers_differ_and_the_losses_read_back(lin_run):
    cases, run, got, before, _ = lin_run
    assert not before[0].any() and not before[1].any() and before[0].size == 16         # no arrays yet: none everywhere
    for w, c in enumerate(cases):
        assert not np.array_equal(run[0][w][0][0], run[1][w][0][0])
        li, lk = got[w]
        assert li.size == 16
        np.testing.assert_array_equal(li[:9], c["loss"])
        np.testing.assert_array_equal(lk[:9], np.where(c["loss"] == R.NONE, 0.0, c["k"]))
        assert not li[9:].any() and not lk[9:].any()
        for which in (0, 1):            # an empty entry reads as zeros
            for arr in run[which][w][1]:
                assert not arr[9:].any()


def test_far_errors_are_rho(lin_run):
    """vf_engine_read_far_errors gives rho(s) for a robust far entry, at the bar rule of test_gpu_robust.py's test_factor_errors_are_rho"""
    cases, run, _, _, errs = lin_run
    rows = _figures(cases, run, 0)
    S = max(x["S"] for x in rows if not R.near_threshold(x["loss"], x["ratio"]))
    for w, c in enumerate(cases):
        fe, fl = errs[w]
        r = run[0][w][0][0]
        assert (fl == -1).all() and (fe[9:] == -1).all()
        for f in range(9):
            loss, k = int(c["loss"][f]), float(c["k"][f])
            with R.mp.workdps(R.DPS):
                s = R.mp.sqrt(sum(R.mp.mpf(float(x)) ** 2 for x in r[f]))
                rho = R.mp_rho(loss, k, s)
                e = float(abs(R.mp.mpf(float(fe[f])) - rho) / rho) if rho != 0 else (0.0 if fe[f] == 0.0 else math.inf)
            x = [y for y in rows if y["w"] == w and y["f"] == f][0]
            b16 = 16 * _own_S(S, x)
            bar = 2 * b16 + b16 * b16 + 4 * R.EPS
            print(f"window {w} entry {f}: {R.NAMES[loss]:14s} error {fe[f]:.6e}, off by {e:.3e} = {e / bar:.3f} of the bar {bar:.2e}")
            assert e <= bar, (w, f)


# ---------------------------------------------------------------- 3. optimum, 4. forms
def run_opt(loss, form=None, trials=F.OPT_TRIALS, shift=False, lossless=False, **kw):
    cases = F.opt_cases(loss)
    eng = make_engine(**kw)
    if form is not None:
        assert eng.solve_form() == form, eng.solve_form()
    for w, c in enumerate(cases[:eng.windows]):
        load(eng, w, c["prob"], c["start"])
        if lossless:
            set_far(eng, w, c)
        else:
            set_far(eng, w, c, np.roll(c["loss"], 1) if shift else c["loss"], np.roll(c["k"], 1) if shift else c["k"])
    eng.iterate(trials)
    out = snapshot(eng)
    eng.close()
    return cases, out


def check_opt(oracle, loss, cases, out, what=""):
    S = F.S_all()
    assert S < 1e-6, S
    bar = 16 * S
    figures = []
    for w, (x, lm) in enumerate(out):
        c, o = cases[w], F.optima(loss, w)
        e = R.position_error(x, o["irls"])
        ad = F.addends(oracle, c, x, c["loss"], c["k"])
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
    """OPT_TRIALS LM trials at the default tuning against the dense host IRLS optimum (GTSAM's form, not the kernel's) at 16 S;
    vf_engine_read_lm's cost against the host's sum of rho at the returned states"""
    cases, out = run_opt(loss)
    check_opt(oracle, loss, cases, out)


FORMS = {
    "one_wave": ("one_wave", dict(chunks=1, sweep_two_sided_max=0, solve_assemble_min=0, solve_split_min=0)),
    "partitioned": ("partitioned", dict(chunks=2)),
    "refined": (None, dict(refine_iterations=2)),
    "gtsam_accept_rule": (None, dict(min_model_fidelity=1e-3)),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_solve_form_consumes_it(oracle, form):
    name, kw = FORMS[form]
    cases, out = run_opt(R.HUBER, form=name, **kw)
    check_opt(oracle, R.HUBER, cases, out, form)


def test_batched_columns_and_big_forms_give_the_same_bits():
    # the Woodbury columns of a single-window engine as one batch: the sequential ones bit for bit
    seq_, bat = (run_opt(R.CAUCHY, trials=6, windows=1, chunks=2, far_batch_columns=x)[1] for x in (0, 1))
    same_snapshots(seq_, bat)
    # the device-memory forms on three entries: the LDS forms bit for bit
    lds, big = (run_opt(R.CAUCHY, trials=6, max_far_factors=16, far_big_forms=x)[1] for x in (0, 1))
    same_snapshots(lds, big)
    # ... and none of them is the run without losses
    assert differ(lds, run_opt(R.CAUCHY, trials=6, max_far_factors=16, lossless=True)[1])
    assert differ(seq_, run_opt(R.CAUCHY, trials=6, windows=1, chunks=2, far_batch_columns=0, lossless=True)[1])


# ---------------------------------------------------------------- 5. nothing asked, nothing changed
def _three_trials(prepare, trials=3):
    cases = F.opt_cases(R.HUBER)
    eng = make_engine()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["start"])
    prepare(eng, cases)
    eng.iterate(trials)
    out = snapshot(eng)
    eng.close()
    return out


def test_nothing_changes_when_nothing_is_asked():
    def plain(eng, cases):
        for w, c in enumerate(cases):
            set_far(eng, w, c)

    def none(eng, cases):                 # the robust call with VF_LOSS_NONE everywhere
        for w, c in enumerate(cases):
            set_far(eng, w, c, [0, 0, 0], [1.0, 2.0, 3.0])

    def huge(eng, cases):                 # Huber with a threshold nothing reaches: the arrays exist, the robust kernel runs
        for w, c in enumerate(cases):
            set_far(eng, w, c, [1, 1, 1], [1e300, 1e300, 1e300])
        assert eng.get_extra_between_loss(0)[0][:3].tolist() == [1, 1, 1]

    def band(eng, cases):                 # band losses (inert: a threshold nothing reaches) and Gaussian far factors
        for w, c in enumerate(cases):
            set_far(eng, w, c)
            eng.set_between_loss(w, c["prob"]["btw_b"] + S0, "huber", 1e30)

    def robust(eng, cases):
        for w, c in enumerate(cases):
            set_far(eng, w, c, c["loss"], c["k"])

    ref = _three_trials(plain)
    for prep in (none, huge, band):
        same_snapshots(ref, _three_trials(prep))
    a, b = _three_trials(robust), _three_trials(robust)
    same_snapshots(a, b)
    assert differ(a, ref)


# ---------------------------------------------------------------- 6. list semantics
def test_list_semantics_and_refusals():
    cases = F.opt_cases(R.HUBER)
    eng = make_engine()
    for w, c in enumerate(cases):
        load(eng, w, c["prob"], c["start"])
        set_far(eng, w, c)
    for w, c in enumerate(cases):
        set_far(eng, w, c, [1 + (w + f) % 3 for f in range(3)], [0.5 + w + 0.25 * f for f in range(3)])
    for w in range(B):
        li, lk = eng.get_extra_between_loss(w)
        assert li.tolist() == [1 + (w + f) % 3 for f in range(3)] + [0] * 5 and lk.tolist() == [0.5 + w + 0.25 * f for f in range(3)] + [0.0] * 5
    set_far(eng, 1, cases[1])                                              # a plain re-send clears window 1's losses, and only those
    assert not eng.get_extra_between_loss(1)[0].any() and not eng.get_extra_between_loss(1)[1].any()
    assert eng.get_extra_between_loss(0)[0][:3].tolist() == [1, 2, 3] and eng.get_extra_between_loss(2)[0][:3].tolist() == [3, 1, 2]
    # refusals touch nothing
    a, b, rec = cases[0]["far"]
    a, b = np.ascontiguousarray(a + S0, dtype=np.int32), np.ascontiguousarray(b + S0, dtype=np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    kept = eng.get_extra_between(0)

    def call(loss, k, e=eng, window=0):
        li, kk = np.array(loss, dtype=np.int32), np.array(k, dtype=np.float64)
        return e._l.vf_engine_set_extra_between_robust(e._h, window, 3, ip(a), ip(b), dp(rec), ip(li), dp(kk))
    for loss, k in (([1, 4, 0], [1.0, 1.0, 1.0]), ([-1, 0, 0], [1.0, 1.0, 1.0]), ([1, 2, 0], [1.0, 0.0, 1.0]), ([1, 2, 0], [-1.0, 1.0, 1.0]),
                    ([3, 0, 0], [math.inf, 1.0, 1.0]), ([0, 0, 2], [1.0, 1.0, math.nan])):
        assert call(loss, k) == -1, (loss, k)
    assert call([1, 0, 0], [1.0, -5.0, math.nan], window=B) == -1           # (k is ignored for VF_LOSS_NONE: the window is refused)
    assert eng.get_extra_between_loss(0)[0][:3].tolist() == [1, 2, 3] and eng.get_extra_between_loss(0)[1][:3].tolist() == [0.5, 0.75, 1.0]
    for x, y in zip(kept[:3], eng.get_extra_between(0)[:3]):
        np.testing.assert_array_equal(x, y)
    assert call([0, 0, 0], [0.0, -1.0, math.nan]) == 0                       # ... and accepted for VF_LOSS_NONE
    eng.close()
    # a time-sharded engine takes no far loss, and an engine that holds far losses is not sharded
    from vil_sensor_fusion_amd import VilFusionError
    sh = make_engine(windows=1, chunks=4)
    sh.set_shard(0, 2)
    assert call([1, 0, 0], [1.0, 1.0, 1.0], e=sh) == -1
    sh.close()
    holds = make_engine(windows=1, chunks=4)
    load(holds, 0, cases[0]["prob"], cases[0]["start"])
    set_far(holds, 0, cases[0], cases[0]["loss"], cases[0]["k"])
    with pytest.raises(VilFusionError) as ei:
        holds.set_shard(0, 2)
    assert ei.value.code == -1
    holds.close()


def _travel(kind, losses_first, shift=False):
    """an engine whose far list travels -- compact + grow, or a re-anchoring slide -- with the losses given BEFORE the journey
    (losses_first) or put directly on the list as it stands after it; three trials"""
    c = F.opt_cases(R.GM)[0]
    w = 0
    seq_prob = F.problem(__import__("oracle.oracle", fromlist=["oracle"]), w, n=N + 1)
    far = F.far_list(w, F.PAIRS, n=N + 1)
    far[2][0, 4:7] += np.array([6.0, -3.0, 1.5])          # (a false match on the first closure, as in the optimum cases)
    case = dict(prob=seq_prob, far=far)
    loss, k = (np.roll(c["loss"], 1), np.roll(c["k"], 1)) if shift else (c["loss"], c["k"])
    s0 = 64 if kind == "compact_grow" else S0
    eng = make_engine(windows=1)
    load(eng, 0, seq_prob, seq_prob["states"], s0=s0, n=N)
    if losses_first:
        set_far(eng, 0, case, loss, k, s0=s0)
    else:
        set_far(eng, 0, case, s0=s0)
    if kind == "compact_grow":
        eng.compact(64)
        eng.grow(200)
        lo = 0
    else:
        eng.slide(marginalize=False)
        lo = s0 + 1
    a, b, rec = eng.get_extra_between(0)[:3]
    if not losses_first:
        eng.set_extra_between(0, a, b, rec, loss=list(loss), k=k)
    got = eng.get_extra_between_loss(0)
    eng.iterate(3)
    out = eng.get_states(0, lo, N), eng.read_lm(0), a - lo, b - lo, got
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["compact_grow", "reanchor"])
def test_losses_travel_with_their_entries(kind):
    c = F.opt_cases(R.GM)[0]
    x, lm, a, b, (li, lk) = _travel(kind, True)
    y, lm2, a2, b2, (li2, lk2) = _travel(kind, False)
    print(f"{kind}: list a {a.tolist()} b {b.tolist()} losses {li[:3].tolist()} k {lk[:3].tolist()}")
    # the pair anchored on the dropped keyframe, (0, 6), is re-anchored on the next one; nothing else moves
    want_a = [1, 0, 3] if kind == "compact_grow" else [0, 0, 2]              # window-local, after the window's first keyframe moved on
    want_b = [9, 6, 5] if kind == "compact_grow" else [8, 5, 4]
    assert a.tolist() == want_a and b.tolist() == want_b
    assert li[:3].tolist() == c["loss"].tolist() and lk[:3].tolist() == c["k"].tolist() and not li[3:].any()
    np.testing.assert_array_equal(li, li2)
    np.testing.assert_array_equal(lk, lk2)
    np.testing.assert_array_equal(x, y)
    assert lm == lm2
    assert not np.array_equal(x, _travel(kind, True, shift=True)[0])         # the comparison has teeth


def test_a_marginalising_slide_takes_the_anchored_entry_off_the_list():
    prob = F.problem(__import__("oracle.oracle", fromlist=["oracle"]), 1, n=N + 1)
    far = F.far_list(1, F.PAIRS, n=N + 1)
    eng = make_engine(windows=1)
    load(eng, 0, prob, prob["states"], n=N)
    eng.set_extra_between(0, far[0] + S0, far[1] + S0, far[2], loss=[2, 1, 3], k=[0.7, 1.9, 2.3])
    eng.iterate(4)
    eng.slide(marginalize=True)
    a, b = eng.get_extra_between(0)[:2]
    li, lk = eng.get_extra_between_loss(0)
    assert (a - S0).tolist() == [1, 3] and (b - S0).tolist() == [9, 5]       # (0, 6) was anchored on the keyframe that left: a linear far factor now
    assert li[:2].tolist() == [2, 3] and lk[:2].tolist() == [0.7, 2.3] and not li[2:].any() and not lk[2:].any()
    assert (eng.get_linear_far(0) - S0).tolist() == [6]
    eng.iterate(4)
    assert eng.read_lm(0)["solve_failures"] == 0
    eng.close()


# ---------------------------------------------------------------- 7. marginalisation
def _lagged(mode, slides=4):
    """a 12-keyframe window over a 17-keyframe clip: the closure (0, 6) is marginalised with its anchor by the first slide, three more
    follow.  mode: "gauss" | "inlier" (Huber with a threshold the closure never reaches) | "gm" (Geman-McClure) on a false match
    ("_bad") or on clean data"""
    oracle = __import__("oracle.oracle", fromlist=["oracle"])
    total = N + slides + 1
    prob = F.problem(oracle, 2, n=total)
    a, b, rec = F.far_list(2, ((0, 6), (3, 5)), n=total)
    if mode.endswith("_bad"):
        rec[0, 4:7] += np.array([6.0, -3.0, 1.5])
    eng = make_engine(windows=1)
    load(eng, 0, prob, prob["states"], n=N)
    if mode.startswith("gauss"):
        eng.set_extra_between(0, a + S0, b + S0, rec)
    elif mode == "inlier":
        eng.set_extra_between(0, a + S0, b + S0, rec, loss=[1, 0], k=[1e6, 0.0])
    else:
        eng.set_extra_between(0, a + S0, b + S0, rec, loss=[3, 0], k=[2.0, 0.0])
    eng.iterate(8)
    for _ in range(slides):
        eng.slide(marginalize=True)
        eng.iterate(6)
    out = eng.get_states(0, S0 + slides, N), eng.read_lm(0), eng.get_extra_between_loss(0)
    eng.close()
    return out


def test_marginalisation_keeps_the_weight_of_its_linearisation():
    g, lm_g, _ = _lagged("gauss")
    h, lm_h, (li, _) = _lagged("inlier")
    np.testing.assert_array_equal(g, h)             # a Huber inlier throughout: the Gaussian engine's bits across the marginalisation of its anchor
    assert lm_g == lm_h and lm_g["solve_failures"] == 0 and not li.any()
    clean = g
    bad_g, bad_r = _lagged("gauss_bad")[0], _lagged("gm_bad")[0]
    d_g, d_r = R.position_error(bad_g, clean), R.position_error(bad_r, clean)
    print(f"a false loop closure marginalised with its anchor, final positions against the clean data's: Gaussian {d_g:.3e} m, Geman-McClure {d_r:.3e} m")
    assert d_r < 0.5 * d_g


# ---------------------------------------------------------------- 8. captured launch sequence
def test_a_far_loss_voids_the_captured_launch_sequence():
    c = F.opt_cases(R.CAUCHY)[0]
    outs = []
    for graph in (False, True):
        eng = make_engine(windows=1, use_hip_graph=graph)
        load(eng, 0, c["prob"], c["start"])
        set_far(eng, 0, c)
        eng.iterate(4)
        eng.iterate(4)
        set_far(eng, 0, c, c["loss"], c["k"])
        eng.iterate(4)
        eng.iterate(4)
        outs.append(snapshot(eng))
        if graph:
            enabled, captures, replays = eng.graph_info()
            assert enabled and captures == 2 and replays == 4
        eng.close()
    same_snapshots(*outs)
