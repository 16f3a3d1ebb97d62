"""The marginalisation cases shared by tests/test_marg_mp_host.py (linearisations from the CPU oracle) and
tests/test_gpu_marg_mp.py (the same records and states loaded into an engine, linearisations read back from the device): one
short synth sequence, hand-built between records, perturbed states, and the two ways of turning them into a mp_marg.Case.
Tests only."""
import itertools

import numpy as np

from tests import helpers, mp_marg
from tests import mp_lie as ml
from vil_sensor_fusion_amd import synth
from vil_sensor_fusion_amd.engine import REFERENCE_PRIOR_SIGMAS

N_SEQ = 80
SUBSETS = [s for k in range(4) for s in itertools.combinations((1, 2, 3), k)]       # the eight subsets of {1, 2, 3}
WEAK_PRIOR_SIGMAS = np.array([1.0] * 3 + [50.0] * 3 + [1e-5] * 3 + [1e-7] * 6)      # gauge information 4e-4 < floor_p of a 6-keyframe window
GRAVITY = np.array([0.0, 0.0, -9.81])
# span patterns: window w holds subset SUBSETS[w] at the leaving keyframe SPAN_LO[w] of a window of SPAN_N[w] keyframes -- on the
# device first slots on both sides of a J-stream tile (8 slots) and of an AoSoA tile (64 slots), a window of exactly 4 and one of
# 5; on the host lo only picks the stretch of the sequence
SPAN_LO = [6, 7, 62, 63, 64, 6, 7, 63]
SPAN_N = [8, 4, 5, 12, 6, 7, 9, 10]
# anchor prior, then three rounds with the previous marginal prior: the spans leaving keyframe CHAIN_LO + k carries (no two
# factors end at the same keyframe: the engine files a between factor under the keyframe it ends at)
CHAIN_LO, CHAIN_N = 62, 9
CHAIN_SUBSETS = [(1, 2), (3,), (1,), (2, 3)]
CHAIN_SCALES = (0.01, 0.5)


def base_problem(oracle):
    """IMU records, initial values and ground truth of the one sequence every case is cut from"""
    seq = synth.make_sequence(seed=977, n_kf=N_SEQ)
    prob = helpers.build_problem(oracle, seq)
    return dict(prob, gt=seq.gt_states, btw_a=np.zeros(0, np.int32), btw_b=np.zeros(0, np.int32), btw=np.zeros((0, 28)))


def between_record(gt, a, b, rng, cov):
    """28-double record of a between factor a -> b: the true relative pose plus noise, a full upper-triangular square-root
    information (off-diagonal entries, so that a row or column in the wrong place changes the result)"""
    Ra, Rb = synth.quat_to_rot(gt[a, 0:4]), synth.quat_to_rot(gt[b, 0:4])
    Rab = Ra.T @ Rb @ synth.so3_exp(rng.normal(size=3) * 1e-3)
    tab = Ra.T @ (gt[b, 4:7] - gt[a, 4:7]) + rng.normal(size=3) * 1e-2
    R = np.triu(rng.normal(size=(6, 6)) * 0.2 / np.sqrt(cov), 1) + np.eye(6) / np.sqrt(cov)
    return np.concatenate([synth.rot_to_quat(Rab), tab, R[np.triu_indices(6)]])


def span_factors(prob, lo, subset, seed):
    """[(d, record)] for the between factors lo -> lo + d, d in subset"""
    rng = np.random.default_rng([seed, lo] + list(subset))
    return [(d, between_record(prob["gt"], lo, lo + d, rng, 1e-4 if d % 2 else 1e-6)) for d in subset]


def perturbed(oracle, states, scale, seed):
    rng = np.random.default_rng([seed, int(scale * 1e6)])
    return np.array([oracle.retract(s, rng.normal(size=15) * scale) for s in states])


def with_spans(prob, placed):
    """prob with the between factors [(lo, [(d, record)])]"""
    a = np.array([lo for lo, fs in placed for _ in fs], dtype=np.int32)
    b = np.array([lo + d for lo, fs in placed for d, _ in fs], dtype=np.int32)
    rec = np.array([r for _, fs in placed for _, r in fs]).reshape(-1, 28)
    return dict(prob, btw_a=a, btw_b=b, btw=rec)


def span_inputs(oracle, prob, i):
    """(lo, n, states of lo .. lo+3, factors, prior record) of span pattern i: anchor prior with the reference sigmas, the
    states 0.01 off its mean"""
    lo = SPAN_LO[i]
    st = perturbed(oracle, prob["states"][lo:lo + 4], 0.01, 100 + i)
    return lo, SPAN_N[i], st, span_factors(prob, lo, SUBSETS[i], 7), reference_prior(prob["states"][lo])


def weak_inputs(oracle, prob):
    """(lo, n, states, factors, prior record) of the case whose anchor prior knows less about the gauge than the floor"""
    lo, n = 6, 6
    st = perturbed(oracle, prob["states"][lo:lo + 4], 0.01, 300)
    return lo, n, st, span_factors(prob, lo, (1, 3), 9), synth.prior_record(prob["states"][lo], WEAK_PRIOR_SIGMAS)


def chain_inputs(oracle, prob, scale, k):
    """(lo, states of lo .. lo+3, factors) of round k (0 = the anchor prior's) of the chain perturbed by `scale`"""
    lo = CHAIN_LO + k
    return lo, perturbed(oracle, prob["states"][lo:lo + 4], scale, 200 + k), span_factors(prob, lo, CHAIN_SUBSETS[k], 8)


# ---------------------------------------------------------------- Case from the oracle's linearisations (host)
def host_case(oracle, name, st4, imu_rec, factors, prior_rec=None, marg=None, n_kf=4):
    r, J = oracle.imu_factor(imu_rec, GRAVITY, st4[0], st4[1])
    btw = []
    for d, rec in factors:
        rb, Ja, Jb = oracle.between_factor(rec, st4[0], st4[d])
        btw.append(dict(d=d, r=rb, Ja=Ja, Jb=Jb))
    prior = None
    if prior_rec is not None:
        rp, Jp = oracle.prior_factor(prior_rec, st4[0])
        prior = dict(r=rp, J=Jp, sig=prior_rec[16:31], rounded=False)
    return mp_marg.Case(name, (r, J), btw, prior, marg, np.array(st4[:4]), n_kf, tuple(GRAVITY))


def oracle_marginalize(oracle, st4, imu_rec, factors, prior_rec=None, marg=None, floor_p=0.0):
    """the C oracle on the same inputs: dict(L, eta, xbar)"""
    pk = np.array([0], dtype=np.int32) if prior_rec is not None else np.zeros(0, dtype=np.int32)
    pd = prior_rec.reshape(1, -1) if prior_rec is not None else np.zeros((0, 31))
    w = oracle.Window(st4[:4], [0], [1], imu_rec.reshape(1, -1), [0] * len(factors), [d for d, _ in factors],
                      np.array([r for _, r in factors]).reshape(-1, 28), pk, pd, GRAVITY)
    if marg is not None:
        m = oracle.Marg()
        m.on, m.k0 = 1, 0
        m.xbar[:] = list(np.asarray(marg["xbar"]).ravel())
        m.L[:] = list(np.asarray(marg["L"]).ravel())
        m.eta[:] = list(np.asarray(marg["eta"]).ravel())
        w.set_marg(m)
    return w.marginalize(0, floor_p).arrays()


# ---------------------------------------------------------------- Case from what the device holds (gpu)
def device_case(eng, w, lo, name, spans, prior_rec=None, marg=None, n_kf=4, absorbed=()):
    """spans: the d of the band between factors lo -> lo + d; prior_rec: the anchor prior's record (its rows come from
    mp_lie.prior_factor, the device's have no reader); marg: read_marginal before this marginalisation;
    absorbed: [(d, record)] far factors lo -> lo + d the prior absorbs (linearised by mp_lie.between_factor)"""
    st = eng.get_states(w, lo, 4)
    r, J = eng.read_imu_lin(w, lo + 1, 1)
    btw = []
    for d in spans:
        rb, Ja, Jb = eng.read_between_lin(w, lo + d, 1)
        btw.append(dict(d=d, r=rb[0], Ja=Ja[0], Jb=Jb[0]))
    for d, rec in absorbed:
        rb, Ja, Jb = ml.between_factor(rec, st[0], st[d])
        btw.append(dict(d=d, r=rb, Ja=Ja, Jb=Jb, rounded=True, R=ml.to_np(ml.upper(ml.vec(rec[7:28]), 6))))
    prior = None
    if prior_rec is not None:
        rp, Jp = ml.prior_factor(prior_rec, st[0])
        prior = dict(r=rp, J=Jp, sig=prior_rec[16:31], rounded=True)
    return mp_marg.Case(name, (r[0], J[0]), btw, prior, marg, st, n_kf, tuple(GRAVITY))


def reference_prior(state):
    return synth.prior_record(state, REFERENCE_PRIOR_SIGMAS)
