"""-m gpu: the per-axis subsets, the four variants (jensen_bregman_0, kullback_leibler_0pose, kullback_leibler_0cov,
condition_cov) and the fused several-subsets launch (vf_degeneracy_scores_batch) of K6, against the reference's own
outputs (tests/golden/degeneracy_axes_golden.npz) and, bit for bit, against the single-subset launches."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "degeneracy_axes_golden.npz"))
NAMES = [str(n) for n in GOLD["names"]]
AXES = ["x", "y", "z", "roll", "pitch", "yaw"]
SUBSETS = ["all", "trans", "rot"] + AXES
KINDS = ["well", "illcond", "tunnel"]
RTOL = {"well": 1e-8, "illcond": 1e-4, "tunnel": 1e-5}      # as tests/test_gpu_degeneracy.py, for the 6x6 / 3x3 blocks


def axis_atol(mats, pose, axis, name):
    """0, except for kullback_leibler(_0pose): 0.5 (r - 1 + du^2 / a - log r) with r = prev / now is a sum of O(1) terms that
    cancels to ~1e-6 where consecutive entries are close, so the reference's own value carries a few ulps of the terms as
    absolute error (numpy's det is exp(log|.|), its log is not the device's): the tolerance is 8 ulps of the terms"""
    if name not in ("kullback_leibler", "kullback_leibler_0pose"):
        return 0.0
    k = AXES.index(axis)
    a, b = mats[k, k, 1:], mats[k, k, :-1]
    du = 0.0 if name.endswith("0pose") else pose[k, 0, :-1] - pose[k, 0, 1:]
    with np.errstate(all="ignore"):
        terms = np.abs(b / a) + 1.0 + du * du / np.abs(a) + np.abs(np.log(np.abs(a) / np.abs(b)))
    atol = np.concatenate([[0.0], 8 * np.finfo(np.float64).eps * terms])
    return np.where(np.isfinite(atol), atol, 0.0)


def same_bits(a, b):
    """equal values, NaN where NaN, and the same sign of every zero"""
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    fin = ~np.isnan(a)
    return np.array_equal(a[fin].view(u), b[fin].view(u))


@pytest.mark.parametrize("kind", KINDS)
def test_per_axis_matches_reference(kind):
    """a 1x1 has no conditioning to excuse: every function, every axis, rtol 1e-12 (kullback_leibler: + 8 ulps of its terms),
    through both entry points"""
    from vil_sensor_fusion_amd import degeneracy as dg
    mats, pose = GOLD[f"{kind}_mats"], GOLD[f"{kind}_pose"]
    for name in NAMES:
        fused = dg.scores(mats, pose, name, subsets=AXES)
        for axis in AXES:
            ref = GOLD[f"{kind}_{axis}"][NAMES.index(name)]
            y = dg.apply_degen_function(mats, pose, axis, name)
            assert y[0] == 0.0
            atol = axis_atol(mats, pose, axis, name)
            assert (np.abs(y - ref) <= 1e-12 * np.abs(ref) + atol)[np.isfinite(ref)].all(), f"{kind}/{axis}/{name}"
            np.testing.assert_allclose(y, ref, rtol=1e-12, atol=np.max(atol), equal_nan=True, err_msg=f"{kind}/{axis}/{name}")
            assert same_bits(fused[axis], y), f"{kind}/{axis}/{name}"


def test_edge_entries_match_reference():
    """zero, negative and tiny diagonal entries: value and NaN / +-inf placement of every function the reference
    evaluates; where it raised (norm_*_ratio of a zero previous entry) the output is not finite"""
    from vil_sensor_fusion_amd import degeneracy as dg
    mats, pose = GOLD["edge_mats"], GOLD["edge_pose"]
    raised = {str(n) for n in GOLD["edge_raised"]}
    for axis in AXES:
        for j, name in enumerate(NAMES):
            ref = GOLD[f"edge_{axis}"][j]
            y = dg.apply_degen_function(mats, pose, axis, name)
            ok = np.ones(ref.shape, bool)
            if name in raised:
                ok = ~np.isnan(ref)
                assert not np.isfinite(y[~ok]).any(), f"{axis}/{name}"
            atol = axis_atol(mats, pose, axis, name)
            with np.errstate(invalid="ignore"):         # inf - inf where both are inf: compared by assert_allclose below
                close = np.abs(y - ref) <= 1e-12 * np.abs(ref) + atol
            assert close[np.isfinite(ref)].all(), f"edge/{axis}/{name}"
            np.testing.assert_allclose(y[ok], ref[ok], rtol=1e-12, atol=np.max(atol), equal_nan=True, err_msg=f"edge/{axis}/{name}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sub", ["all", "trans", "rot"])
def test_variants_match_reference(kind, sub):
    from vil_sensor_fusion_amd import degeneracy as dg
    mats, pose = GOLD[f"{kind}_mats"], GOLD[f"{kind}_pose"]
    for name in dg.EXTRA_METRICS:
        ref = GOLD[f"{kind}_{sub}"][NAMES.index(name)]
        y = dg.apply_degen_function(mats, None, sub, name)
        assert y[0] == 0.0
        if name == "kullback_leibler_0cov":
            assert np.isnan(ref[1:]).all() and np.isnan(y[1:]).all()
            continue
        if name == "kullback_leibler_0pose" and (kind == "illcond" or (kind == "tunnel" and sub != "rot")):
            continue        # inv(now) @ prev with kappa^2 >> 1/eps: the reference's own value is rounding noise
        if name == "condition_cov" and kind == "illcond":
            np.testing.assert_allclose(y, ref, rtol=5e-3)        # kappa * eps, as condition_number
            continue
        scale = np.abs(ref).max()
        np.testing.assert_allclose(y, ref, rtol=RTOL[kind], atol=RTOL[kind] * scale * 1e-3, err_msg=f"{kind}/{sub}/{name}")


def _inputs():
    rng = np.random.default_rng(2026)
    T = 20011                                   # not a multiple of 64: the last wave is partial
    A = rng.normal(size=(T, 6, 6))
    mats = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(6)
    pose = rng.normal(size=(T, 6))
    out = [(GOLD[f"{k}_mats"], GOLD[f"{k}_pose"]) for k in KINDS + ["edge"]]
    out.append((np.ascontiguousarray(mats.transpose(1, 2, 0)), np.ascontiguousarray(pose.T[:, None, :])))
    return out


def test_condition_cov_is_negated_condition_number():
    """bit for bit, on the symmetric eigen path, on the SVD path (a batch that is not symmetric) and on the 1x1 path"""
    from vil_sensor_fusion_amd import degeneracy as dg
    nonsym = np.ascontiguousarray(np.tile(np.triu(np.arange(1.0, 37.0).reshape(6, 6))[:, :, None], (1, 1, 70)))
    for mats, _ in _inputs()[:4] + [(nonsym, None)]:
        for sub in SUBSETS:
            for dt in (np.float64, np.float32):
                cn = dg.apply_degen_function(mats, None, sub, "condition_number", dtype=dt)
                cc = dg.apply_degen_function(mats, None, sub, "condition_cov", dtype=dt)
                assert same_bits(cc[1:], -cn[1:]), sub
    cc = dg.apply_degen_function(nonsym, None, "all", "condition_cov")
    np.testing.assert_allclose(cc[1:], np.linalg.cond(nonsym[:, :, 1]), rtol=1e-9)


def test_kullback_leibler_0pose_is_kullback_leibler_at_zero_pose():
    from vil_sensor_fusion_amd import degeneracy as dg
    for mats, pose in _inputs()[:4]:
        zero = np.zeros_like(pose)
        for sub in SUBSETS:
            for dt in (np.float64, np.float32):
                a = dg.apply_degen_function(mats, None, sub, "kullback_leibler_0pose", dtype=dt)
                b = dg.apply_degen_function(mats, zero, sub, "kullback_leibler", dtype=dt)
                assert same_bits(a, b), sub


def test_fused_equals_separate():
    """vf_degeneracy_scores_batch: every row bit for bit the single-subset launch, for all 25 metrics, both dtypes and
    masks {all, trans, rot}, all nine, each single subset and a sparse {rot, yaw}"""
    from vil_sensor_fusion_amd import degeneracy as dg
    masks = [("all", "trans", "rot"), tuple(SUBSETS), ("rot", "yaw")] + [(s,) for s in SUBSETS]
    for mats, pose in _inputs():
        for dt in (np.float64, np.float32):
            for name in dg.METRICS + dg.EXTRA_METRICS:
                single = {s: dg.apply_degen_function(mats, pose, s, name, dtype=dt) for s in SUBSETS}
                for mask in masks:
                    got = dg.scores(mats, pose, name, subsets=mask, dtype=dt)
                    for s in mask:
                        assert same_bits(got[s], single[s]), f"{name}/{dt.__name__}/{mask}/{s}"


def test_scores_default_is_the_online_node_shape():
    from vil_sensor_fusion_amd import degeneracy as dg
    mats, pose = GOLD["well_mats"], GOLD["well_pose"]
    got = dg.scores(mats, pose, "d_opt")
    assert list(got) == ["all", "trans", "rot"]
    for s in got:
        assert same_bits(got[s], dg.apply_degen_function(mats, pose, s, "d_opt"))


def test_spectrum_per_axis_is_the_three_metrics():
    from vil_sensor_fusion_amd import degeneracy as dg
    for mats, _ in _inputs()[:4]:
        for axis in AXES:
            for dt in (np.float64, np.float32):
                got = dg.spectrum(mats, axis, dtype=dt)
                for name in ("e_opt", "max_eigen", "condition_number"):
                    assert same_bits(got[name], dg.apply_degen_function(mats, None, axis, name, dtype=dt)), f"{axis}/{name}"
