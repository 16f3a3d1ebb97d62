"""-m gpu: vf_degeneracy_remap_batch / k_remap_covariance against the mpmath reference of tests/remap_ref.py, at the bars
tests/test_remap_ref_host.py fixes (16 x S + 64 eps; nothing of them comes from a device result), and the properties the
entry point promises: exactly nominal where nothing is deweighted, symmetric to the bit, the same bits whatever the batch
around a message, float32 = float64 on the promoted values, the output order a pure permutation, a non-finite Hessian
contained, every argument error refused before anything is written."""
import ctypes as C

import numpy as np
import pytest

from tests import remap_ref as mr
from vil_sensor_fusion_amd import _lib, synth
from vil_sensor_fusion_amd.degeneracy import POSE3_FROM_LOAM, remap_covariance

pytestmark = pytest.mark.gpu

_one = {}


def one(name, thr=None):
    """the device's outputs for one case in a batch of one (cached): (cov (6, 6), sqrt_info (21,), eig (6,), deweighted).
    thr: both thresholds (the batch tests run every matrix at one pair); None: the case's own"""
    if (name, thr) not in _one:
        H, tt, rt = mr.cases()[name]
        tt, rt = (tt, rt) if thr is None else (thr, thr)
        cov, sq, eig, dw = remap_covariance(H[None], mr.NOM6, trans_thr=tt, rot_thr=rt, floor=mr.FLOOR)
        _one[(name, thr)] = (cov[0], sq[0], eig[0], int(dw[0]))
    return _one[(name, thr)]


@pytest.mark.parametrize("name", mr.CASES)
def test_case_within_its_bar(name):
    cov, sq, eig, dw = one(name)
    C_ref, M_ref, E_ref, dw_ref = mr.case_reference(name)
    e = (mr.err(cov, C_ref), mr.err(mr.info_of(sq), M_ref), mr.eig_err(eig, E_ref))
    b = mr.bar(name)
    print(f"case {name}: cov {e[0]:.3e} (bar {b[0]:.3e}), R^T R {e[1]:.3e} (bar {b[1]:.3e}), eig {e[2]:.3e} (bar {b[2]:.3e}), deweighted {dw}")
    assert dw == dw_ref == mr.DEWEIGHTED[name]
    assert np.all(np.diff(eig) >= 0.0)
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2]
    assert cov.tobytes() == cov.T.copy().tobytes()                       # symmetric to the bit
    R = np.zeros((6, 6))
    R[np.triu_indices(6)] = sq
    assert np.all(np.diag(R) > 0.0)


@pytest.mark.parametrize("name", mr.EXACTLY_NOMINAL)
def test_nothing_deweighted_is_the_nominal_bit_for_bit(name):
    cov, sq, _, dw = one(name)
    R = np.zeros((6, 6))
    R[np.triu_indices(6)] = sq
    assert dw == 0
    assert cov.tobytes() == np.diag(mr.NOM6).tobytes()
    assert R.tobytes() == np.diag(1.0 / np.sqrt(mr.NOM6)).tobytes()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_a_message_has_the_bits_of_a_batch_of_one(count):
    """tile edges, a wave with a single live lane (65, 129), and lanes that converge in different sweeps side by side"""
    names = [mr.CASES[(3 * i + count) % len(mr.CASES)] for i in range(count)]
    H = np.stack([mr.cases()[n][0] for n in names])
    cov, sq, eig, dw = remap_covariance(H, mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR)
    assert len(set(names)) == min(count, len(mr.CASES))
    for i, n in enumerate(names):
        c1, s1, e1, d1 = one(n, mr.THR)
        assert cov[i].tobytes() == c1.tobytes() and sq[i].tobytes() == s1.tobytes() and eig[i].tobytes() == e1.tobytes() and dw[i] == d1, (i, n)


def test_float32_is_float64_on_the_promoted_values():
    H32 = np.stack([mr.cases()[n][0] for n in mr.CASES] * 7).astype(np.float32)[:67]
    a = remap_covariance(H32, mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR, dtype=np.float32)
    b = remap_covariance(H32.astype(np.float64), mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR, dtype=np.float64)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert np.any(a[3] > 0) and np.any(a[3] == 0)


def test_pose3_order_is_the_block_permutation():
    H = np.stack([mr.cases()[n][0] for n in mr.CASES])
    P = POSE3_FROM_LOAM
    assert mr.CASES[0] == "open"
    c0, s0, e0, d0 = remap_covariance(H, mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR, order="loam")
    c1, s1, e1, d1 = remap_covariance(H, mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR, order="pose3")
    assert c1.tobytes() == np.ascontiguousarray(c0[:, P][:, :, P]).tobytes()
    assert e1.tobytes() == e0.tobytes() and np.array_equal(d0, d1)
    for i, name in enumerate(mr.CASES):
        if mr.cases()[name][1] != mr.THR:
            continue                                      # (split thresholds: run at THR here, it has no reference at that pair)
        M_ref = mr.case_reference(name)[1][np.ix_(P, P)]
        e = mr.err(mr.info_of(s1[i]), M_ref)
        print(f"case {name}, pose3 order: R^T R {e:.3e} (bar {mr.bar(name)[1]:.3e})")
        assert e <= mr.bar(name)[1]
    # where nothing is deweighted R is the permuted nominal to the bit
    R = np.zeros((6, 6))
    R[np.triu_indices(6)] = s1[0]
    assert R.tobytes() == np.diag(1.0 / np.sqrt(mr.NOM6[P])).tobytes()


def test_a_non_finite_hessian_stays_alone():
    names = [mr.CASES[i % len(mr.CASES)] for i in range(70)]
    H = np.stack([mr.cases()[n][0] for n in names])
    bad = {5: np.nan, 63: np.inf, 64: -np.inf, 69: np.nan}
    for i, v in bad.items():
        H[i, i % 6, (i + 2) % 6] = v
    cov, sq, eig, dw = remap_covariance(H, mr.NOM6, trans_thr=mr.THR, rot_thr=mr.THR, floor=mr.FLOOR)
    for i, n in enumerate(names):
        if i in bad:
            R = np.zeros((6, 6))
            R[np.triu_indices(6)] = sq[i]
            assert dw[i] == -1 and np.all(np.isnan(eig[i]))
            assert cov[i].tobytes() == np.diag(mr.NOM6 / mr.FLOOR).tobytes()
            assert np.array_equal(R, np.diag(np.diag(R))) and mr.err(R.T @ R, np.diag(mr.FLOOR / mr.NOM6)) <= 64 * np.finfo(float).eps
        else:
            c1, s1, e1, d1 = one(n, mr.THR)
            assert cov[i].tobytes() == c1.tobytes() and sq[i].tobytes() == s1.tobytes() and eig[i].tobytes() == e1.tobytes() and dw[i] == d1, (i, n)


def _raw(h, count, dtype, nom, tt, rt, floor, order, cov, sq, eig, dw):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return _lib.lib().vf_degeneracy_remap_batch(p(h), count, dtype, p(nom), tt, rt, floor, order, p(cov), p(sq), p(eig), p(dw), 0, None)


def test_argument_errors_are_refused_before_anything_is_written():
    H = np.ascontiguousarray(np.stack([mr.cases()["tunnel"][0]] * 3))
    nom = mr.NOM6.copy()
    good = dict(h=H, count=3, dtype=0, nom=nom, tt=1e3, rt=1e3, floor=1e-6, order=0)
    bad_nom = nom.copy()
    bad_nom[4] = 0.0
    nan_nom = nom.copy()
    nan_nom[0] = np.nan
    wrong = [dict(h=None), dict(nom=None), dict(count=-1), dict(dtype=2), dict(dtype=-1), dict(order=2), dict(order=-1),
             dict(tt=0.0), dict(tt=-1.0), dict(rt=0.0), dict(rt=float("nan")), dict(floor=0.0), dict(floor=1.5), dict(floor=float("nan")),
             dict(nom=bad_nom), dict(nom=nan_nom), dict(cov=None), dict(dw=None)]
    for w in wrong:
        cov, sq, eig, dw = np.full((3, 36), 7.0), np.full((3, 21), 7.0), np.full((3, 6), 7.0), np.full(3, 7, np.int32)
        args = dict(good, cov=cov, sq=sq, eig=eig, dw=dw)
        args.update(w)
        rc = _raw(**args)
        assert rc == -1, (w, rc)                                   # VF_ERR_INVALID
        assert _lib.lib().vf_last_error().decode() != "", w
        assert np.all(cov == 7.0) and np.all(sq == 7.0) and np.all(eig == 7.0) and np.all(dw == 7), w
    # the optional outputs may be absent; floor = 1 is allowed and leaves every message at the nominal
    cov, dw = np.zeros((3, 36)), np.zeros(3, np.int32)
    assert _raw(**dict(good, cov=cov, sq=None, eig=None, dw=dw)) == 0
    assert cov[0].tobytes() == one("tunnel")[0].tobytes() and np.all(dw == 1)
    assert _raw(**dict(good, floor=1.0, cov=cov, sq=None, eig=None, dw=dw)) == 0
    assert cov[0].tobytes() == np.diag(nom).tobytes() and np.all(dw == 0)
    assert _raw(**dict(good, count=0, cov=cov, sq=None, eig=None, dw=dw)) == 0


def test_synth_hessians_lose_exactly_the_tunnel_direction():
    """default thresholds (those of the shipped gate): one direction let go on every tunnel scan and none elsewhere; there the
    information along the generator's direction v -- the eigenvector of the smallest eigenvalue of the Hessian -- falls below
    1e-3 of the nominal and stays above 0.5 of it along the five other eigen-directions"""
    seq = synth.make_sequence(seed=42, n_kf=300, tunnel=mr.TUNNEL)
    in_tunnel = seq.tunnel[seq.loam_kf]
    cov, sq, eig, dw = remap_covariance(seq.loam_hessians, mr.NOM6)
    assert in_tunnel.sum() >= 20 and (~in_tunnel).sum() >= 20
    np.testing.assert_array_equal(dw, in_tunnel.astype(np.int32))
    Ninv = np.diag(1.0 / mr.NOM6)
    assert cov[~in_tunnel].tobytes() == np.stack([np.diag(mr.NOM6)] * int((~in_tunnel).sum())).tobytes()
    worst_v, worst_w = 0.0, np.inf
    for i in np.nonzero(in_tunnel)[0]:
        lam, V = np.linalg.eigh(seq.loam_hessians[i])
        M = mr.info_of(sq[i])
        ratio = np.array([V[:, k] @ M @ V[:, k] / (V[:, k] @ Ninv @ V[:, k]) for k in range(6)])
        worst_v, worst_w = max(worst_v, ratio[0]), min(worst_w, ratio[1:].min())
        np.testing.assert_allclose(eig[i], lam, rtol=0, atol=1e-12 * lam[-1])
    print(f"tunnel scans: v^T M v / v^T N^-1 v at most {worst_v:.3e} along v, at least {worst_w:.6f} along the others")
    assert worst_v < 1e-3 and worst_w > 0.5
