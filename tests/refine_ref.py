"""References of the refined solve (csrc/vf_refine.hip, engine/engine_solve.inc) at small windows, tests only.  No GPU here.

The refined solve answers  (J^T J + L + lambda I) d = -(J^T r + g_mp)  by conjugate gradients whose operator is applied
THROUGH the whitened Jacobian rows J (k_jv, k_jtu, k_far_apply), preconditioned by the engine's Cholesky solve of the normal
equations.  L, g_mp: the marginal prior, kept in information form on [lo: 15][lo+1: pose][lo+2: pose].  Four things:

  * `rows`: J and r of one window [lo, hi) at given states as DENSE float64, factor by factor from the CPU oracle
    (oracle.imu_factor / between_factor / prior_factor), the 30 GTSAM columns of an IMU factor mapped to (keyframe, tangent
    component) as col_comp / jcol_is_j do on the device; far factors six more rows each; the marginal prior as L and
    g_mp = L d + eta, d = Local(xbar -> x) by oracle/twin_qr.MargPrior.delta.
  * `exact`: the minimiser of |J d + r|^2 + d^T L d + 2 g_mp^T d + lambda |d|^2: float64 Householder QR of
    [J; sqrt(lambda) I; sqrt(max(ev, 0)) V^T] (the last 27 rows from eigh(L): L is semi-definite only to rounding, so they
    serve as a SOLVER, never as the statement), then corrected semi-normal refinement with the gradient
    J^T (J x + r) + L x + g_mp + lambda x evaluated in np.longdouble, until a correction is below 1e-15 of max |d|.
  * `restatement`: the algorithm of engine_solve.inc / vf_refine.hip in plain float64: start M^-1 (-g) with
    M = H + lambda I (oracle.band_solve; H, g from Window.assemble(w=3)) -- with far factors M = H + lambda I + U^T U, its
    inverse by the Woodbury identity around the same band solve --, nres = g + A x, then corrections with the kernels'
    scalars and stopping rule (k_pcg_scalar).
  * `err`: max |x - dref| after dividing each of the 15 tangent components by the largest |dref| of that component over
    the window (rotations, positions, velocities and biases differ in scale by orders of magnitude).

The case table (make_case) and what was measured on it live here too: E_CASE, the restatement's error, and U_CASE, how far
the reference moves with the rounding of its inputs.  The device is held to 16 x E_CASE + 2 x U_CASE; 16 is the project's
margin for two correct float64 evaluations of one formula in different summation orders (tests/propagate_ref.py).
tests/test_refine_ref_host.py is what fixes the numbers."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from scipy.linalg import solve_triangular
from scipy.sparse import csr_matrix

from tests import helpers
from vil_sensor_fusion_amd import synth

LAMBDA, REFINE, REL_STOP = 1e-5, 4, 1e-8       # REL_STOP: the default of vf_engine_opts.refine_rel_stop
BAR_FACTOR = 16.0
IMU_COL_I = list(range(0, 9)) + list(range(18, 24))      # GTSAM column of the 15 x 30 Jacobian for tangent component c of keyframe i
IMU_COL_J = list(range(9, 18)) + list(range(24, 30))     # ... of keyframe j (inverse of col_comp in vf_refine.hip)
FAR = ((5, 60), (5, 33), (12, 69))                        # case F: two slots on keyframe 5, one ending at the last keyframe

# err(restatement, dref) per case as measured by tests/test_refine_ref_host.py (the value beside each constant), rounded up
# to two digits.  The test asserts measured <= written <= 1.25 x measured; the bar is `bar` below.
E_CASE = {
    "A": 2.7e-8,      # measured 2.671e-08 (start 1.611e-07)
    "B": 1.9e-7,      # measured 1.847e-07 (start 1.632e-05)
    "F": 1.7e-8,      # measured 1.676e-08 (start 3.528e-08)
    "M": 4.1e-13,     # measured 4.054e-13 (start 2.880e-08)
}
# does the restatement improve on its start (the unrefined solve) by 8 x or more?  As measured: A gains 6.0 x and F 2.1 x
# (both start within a few times the floor eps |g| |M^-1| that forming the residual as g + J^T (J x) leaves); B gains 88 x
# (the X0 prior on keyframe 3 is far from its state: a large step), M 7e4 x (almost converged: g is small and so is the floor).
IMPROVES_8X = {"A": False, "B": True, "F": False, "M": True}
# How far dref itself moves when its INPUTS are another correct float64 evaluation of the same factors: err(exact(rows whose
# IMU, between and X0-prior residuals and Jacobians come from oracle/twin_qr.py -- autodiff of generic matrix functions --),
# dref), `input_sensitivity` below.  The device linearises with its own kernels, a third such evaluation, so its distance from
# dref has this term whatever vf_refine.hip does, and the bar is BAR_FACTOR x E_CASE + INPUT_FACTOR x U_CASE.  U_CASE is already
# a distance between two correct evaluations, not the error of one: the device's linearisation stands to the oracle's as the
# twin's does, and INPUT_FACTOR = 2 allows it twice that distance.  For A, B and F the term is 1e-4 of the bar or less and the
# bar is 16 x E_CASE as before.  In case M it decides: the window is almost converged, the increment's bias components are
# 1e-7 .. 2e-6, and residuals that differ by 3e-12 (1e-16 of a position, whitened) move them by 2.3e-11 of their size, 57 x
# the restatement's 4.1e-13 -- the restatement shares the oracle's residuals with dref, the device cannot.
U_CASE = {
    "A": 3.8e-14,     # measured 3.768e-14
    "B": 2.2e-12,     # measured 2.144e-12
    "F": 1.3e-14,     # measured 1.210e-14 (the far factors' rows are the oracle's in both)
    "M": 2.4e-11,     # measured 2.329e-11
}


INPUT_FACTOR = 2.0


def bar(case):
    return BAR_FACTOR * E_CASE[case] + INPUT_FACTOR * U_CASE[case]


def mp_index(i):
    """27-vector of the marginal prior -> (keyframe offset from lo, tangent component)"""
    return (0, i) if i < 15 else ((1, i - 15) if i < 21 else (2, i - 21))


MP_COLS = [k * 15 + c for k, c in map(mp_index, range(27))]


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    """one window: prob = helpers.build_problem's dict (every keyframe LOADED, also those outside [lo, hi)), states (n, 16)
    of the loaded keyframes, the X0 prior's keyframe or None, far = (a, b, records) with absolute keyframe numbers,
    marg = dict(L, eta, xbar) or None"""
    name: str
    prob: dict
    states: np.ndarray
    lo: int
    hi: int
    prior_k: int | None
    far: tuple | None = None
    marg: dict | None = None
    slides: int = 0

    @property
    def n(self):
        return self.hi - self.lo


def far_records(seq, pairs, seed=5, cov=0.05, noise=(5e-4, 5e-3)):
    """between records of arbitrary keyframe pairs: the ground truth's relative pose + noise, isotropic covariance"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(pairs), 28))
    iu = np.triu_indices(6)
    for f, (a, b) in enumerate(pairs):
        Ra, Rb = synth.quat_to_rot(seq.gt_states[a, :4]), synth.quat_to_rot(seq.gt_states[b, :4])
        Rab = Ra.T @ Rb @ synth.so3_exp(rng.normal(size=3) * noise[0])
        tab = Ra.T @ (seq.gt_states[b, 4:7] - seq.gt_states[a, 4:7]) + rng.normal(size=3) * noise[1]
        out[f, 0:4], out[f, 4:7] = synth.rot_to_quat(Rab), tab
        out[f, 7 + np.nonzero(iu[0] == iu[1])[0]] = 1.0 / np.sqrt(cov)
    return out


M_SEED, M_N, M_SLIDES, M_TRIALS = 43, 70, 2, 4
# Case M slides TWICE.  The between factors of synth.make_sequence follow the sensors' fixed interleaving (camera, LiDAR,
# camera, camera, LiDAR, ...): span-3 factors start at keyframes 1, 4, 7, ... whatever the seed, so the prior left by
# marginalising keyframe 0 alone has L[21:27] = 0 (nothing couples keyframe 0 to keyframe 3) and a mutation of those rows
# changes nothing.  Marginalising keyframe 1 as well (its factor 1 -> 4) fills them: the window is [2, 72).


# Case A is seed 32, not 0.  Every mutation of tests/test_refine_ref_host.py has to land beyond 10 x the case's bar, a
# condition on the inputs alone.  The weakest mutation is "no lambda" (it moves the increment by ~6e-6 at 70 keyframes whatever
# the seed) and the restatement's own error is a rounding floor that wanders between 1e-8 and 1e-7 with the seed: at seed 0 it
# is 3.5e-8 and "no lambda" lands at 9.97 x the bar.  Of the seeds 0 .. 39 those with 10 x or more are 1, 2, 15, 22, 29, 32,
# 34, 39; 32 has the largest floor among those with a margin (2.7e-8, 14 x), so the bar it gives the device is not a lucky
# one.  Case F keeps seed 0 (1.7e-8, 12.3 x): it is the window case A was meant to be, plus the far factors.


def case_inputs(name):
    """(seed, keyframes loaded, perturb, lo, hi) of a case before any slide"""
    return {"A": (32, 70, 0.01, 0, 70), "F": (0, 70, 0.01, 0, 70), "B": (1, 200, 0.01, 3, 131),
            "M": (M_SEED, M_N + M_SLIDES, 0.0, 0, M_N)}[name]


def problem(oracle, name):
    seed, n, perturb, lo, hi = case_inputs(name)
    seq = synth.make_sequence(seed=seed, n_kf=n)
    return seq, helpers.build_problem(oracle, seq, perturb=perturb)


def make_case(oracle, name) -> Case:
    """the case as the CPU oracle sees it (M: the oracle does the LM trials and the marginalisations itself)"""
    seq, prob = problem(oracle, name)
    _, n, _, lo, hi = case_inputs(name)
    if name == "M":
        fl = helpers.FixedLagOracle(oracle, prob, M_N, M_TRIALS)
        for _ in range(M_SLIDES - 1):
            fl.update()
        marg = fl.win.marginalize(0, oracle.prior_gauge_floor(M_N)).arrays()
        states = fl.states.copy()
        states[M_N + M_SLIDES - 1] = oracle.predict(prob["imu"][M_N + M_SLIDES - 1], prob["gravity"], states[M_N + M_SLIDES - 2])
        return Case("M", prob, states, M_SLIDES, M_N + M_SLIDES, None, marg=dict(L=marg["L"], eta=marg["eta"], xbar=marg["xbar"]), slides=M_SLIDES)
    far = None
    if name == "F":
        far = (np.array([a for a, _ in FAR], dtype=np.int32), np.array([b for _, b in FAR], dtype=np.int32), far_records(seq, FAR))
    return Case(name, prob, prob["states"].copy(), lo, hi, lo, far=far)


# ---------------------------------------------------------------- rows
@dataclass
class Rows:
    """J (m, 15 n), r (m,), L (15 n, 15 n) and g_mp (15 n,) (zero without a marginal prior), and where every factor's rows
    are: blocks = [(kind, a, b, first row, rows)] with window-local keyframes (kind: imu, btw, prior, far)"""
    J: np.ndarray
    r: np.ndarray
    L: np.ndarray
    g_mp: np.ndarray
    blocks: list = field(default_factory=list)

    def find(self, kind, a=None, b=None):
        return [blk for blk in self.blocks if blk[0] == kind and (a is None or blk[1] == a) and (b is None or blk[2] == b)]


def marg_gradient(marg, states_lo3):
    """L d + eta with d = Local(xbar -> x) of the three keyframes the prior sits on (twin_qr.MargPrior.delta)"""
    from oracle import twin_qr
    mp = twin_qr.MargPrior(0, twin_qr.States.from_array(marg["xbar"]), np.zeros((0, 27)), np.zeros(0))
    d = mp.delta(twin_qr.States.from_array(states_lo3))
    return marg["L"] @ d + marg["eta"]


def rows(oracle, case: Case) -> Rows:
    lo, hi, n, st, p = case.lo, case.hi, case.n, case.states, case.prob
    Js, rs, blocks = [], [], []
    m = 0

    def add(kind, a, b, r, cols):
        nonlocal m
        J = np.zeros((r.size, 15 * n))
        for k, Jk in cols:
            J[:, 15 * k:15 * k + Jk.shape[1]] = Jk
        Js.append(J); rs.append(r); blocks.append((kind, a, b, m, r.size))
        m += r.size

    for k in range(lo + 1, hi):
        r, J = oracle.imu_factor(p["imu"][k], p["gravity"], st[k - 1], st[k])
        add("imu", k - 1 - lo, k - lo, r, [(k - 1 - lo, J[:, IMU_COL_I]), (k - lo, J[:, IMU_COL_J])])
    for a, b, rec in zip(p["btw_a"], p["btw_b"], p["btw"]):
        if a >= lo and b < hi:                   # both ends inside the range (factors outside stay in the engine's slots)
            r, Ja, Jb = oracle.between_factor(rec, st[a], st[b])
            add("btw", a - lo, b - lo, r, [(a - lo, Ja), (b - lo, Jb)])
    if case.prior_k is not None:
        r, J = oracle.prior_factor(p["prior"], st[case.prior_k])      # helpers.load_engine puts the SAME record on keyframe lo
        add("prior", case.prior_k - lo, case.prior_k - lo, r, [(case.prior_k - lo, J)])
    if case.far is not None:
        for a, b, rec in zip(*case.far):
            r, Ja, Jb = oracle.between_factor(rec, st[a], st[b])
            add("far", a - lo, b - lo, r, [(a - lo, Ja), (b - lo, Jb)])
    L, g_mp = np.zeros((15 * n, 15 * n)), np.zeros(15 * n)
    if case.marg is not None:
        L[np.ix_(MP_COLS, MP_COLS)] = case.marg["L"]
        g_mp[MP_COLS] = marg_gradient(case.marg, st[lo:lo + 3])
    return Rows(np.vstack(Js), np.concatenate(rs), L, g_mp, blocks)


# ---------------------------------------------------------------- exact
def exact(rw: Rows, lam, max_steps=6, tol=1e-15):
    """(d (n, 15), size of the last correction relative to max |d|, sizes of all corrections)"""
    N = rw.J.shape[1]
    stack = [rw.J, np.sqrt(lam) * np.eye(N)]
    if np.any(rw.L):
        ev, V = np.linalg.eigh(rw.L[np.ix_(MP_COLS, MP_COLS)])
        S = np.zeros((27, N))
        S[:, MP_COLS] = np.sqrt(np.maximum(ev, 0.0))[:, None] * V.T
        stack.append(S)
    Rf = np.linalg.qr(np.vstack(stack), mode="r")          # LAPACK geqrf: Householder reflections, no normal equations
    Jl, rl, Ll, gl = (a.astype(np.longdouble) for a in (rw.J, rw.r, rw.L, rw.g_mp))
    has_L = bool(np.any(rw.L))
    x = np.zeros(N, dtype=np.longdouble)
    sizes = []
    for _ in range(max_steps + 1):                         # the first pass is the semi-normal solution itself
        grad = Jl.T @ (Jl @ x + rl) + gl + np.longdouble(lam) * x
        if has_L:
            grad = grad + Ll @ x
        dx = -solve_triangular(Rf, solve_triangular(Rf, np.asarray(grad, dtype=np.float64), trans="T"))
        x = x + dx.astype(np.longdouble)
        sizes.append(float(np.max(np.abs(dx)) / np.max(np.abs(x))))
        if len(sizes) > 1 and sizes[-1] < tol:
            break
    return np.asarray(x, dtype=np.float64).reshape(-1, 15), sizes[-1], sizes[1:]


# ---------------------------------------------------------------- restatement
def marg_struct(oracle, marg):
    """oracle.Marg (k0 = 0: window-local) from dict(L, eta, xbar)"""
    m = oracle.Marg()
    m.on, m.k0 = 1, 0
    m.xbar[:] = list(np.asarray(marg["xbar"], dtype=np.float64).ravel())
    m.L[:] = list(np.asarray(marg["L"], dtype=np.float64).ravel())
    m.eta[:] = list(np.asarray(marg["eta"], dtype=np.float64).ravel())
    return m


def normal_equations(oracle, case: Case):
    """(H (n, 4, 15, 15), g (n, 15)) of the band part -- IMU, between, X0 prior, marginal prior -- by Window.assemble(w=3)"""
    lo, hi, p = case.lo, case.hi, case.prob
    sel = (p["btw_a"] >= lo) & (p["btw_b"] < hi)
    ks = np.arange(lo + 1, hi)
    pk = np.zeros(0, dtype=np.int32) if case.prior_k is None else np.array([case.prior_k - lo], dtype=np.int32)
    pd = np.zeros((0, 31)) if case.prior_k is None else p["prior"].reshape(1, -1)
    win = oracle.Window(case.states[lo:hi], ks - 1 - lo, ks - lo, p["imu"][lo + 1:hi], p["btw_a"][sel] - lo, p["btw_b"][sel] - lo,
                        p["btw"][sel], pk, pd, p["gravity"])
    keep = None
    if case.marg is not None:
        keep = marg_struct(oracle, case.marg)
        win.set_marg(keep)
    _, H, g = win.assemble(w=3)
    return H, g


def band_dense(H):
    """the symmetric (15 n, 15 n) matrix of a band H[k][d] = block (k, k - d)"""
    n, w1 = H.shape[0], H.shape[1]
    D = np.zeros((15 * n, 15 * n))
    for k in range(n):
        for d in range(min(w1, k + 1)):
            D[15 * k:15 * k + 15, 15 * (k - d):15 * (k - d) + 15] = H[k, d]
            if d:
                D[15 * (k - d):15 * (k - d) + 15, 15 * k:15 * k + 15] = H[k, d].T
    return D


def operator(rw: Rows, lam):
    """A p = J^T (J p) + L p + lambda p.  The products are scipy's sparse ones: a plain loop over the stored entries in index
    order, the same bits on every host (a BLAS product's summation order changes with the library and its thread count, and
    the figures below sit at the rounding floor)"""
    J, Jt, L = csr_matrix(rw.J), csr_matrix(np.ascontiguousarray(rw.J.T)), csr_matrix(rw.L)
    return lambda p: Jt @ (J @ p) + L @ p + lam * p


def preconditioner(oracle, case: Case, rw: Rows, lam=LAMBDA, normal=None):
    """(v -> M^-1 v, g (15 n,), H band, U dense or None): M = H + lambda I + U^T U, U the far factors' rows; g with their
    J^T r.  The band part is oracle.band_solve; normal = (H, g) is another evaluation of it than normal_equations
    (tests/direct_ref.py).  With far factors M^-1 v = y - Z (I + U Z)^-1 U y, y = B^-1 v, Z = B^-1 U^T,
    B = H + lambda I: the inverse of the dense M (tests/test_refine_ref_host.py holds it to that), evaluated the way the
    engine does and without BLAS -- a LAPACK Cholesky of the dense M changes its summation order with the thread count, and
    case F's figure with it (1.77e-8 with eight threads, 1.34e-8 with one)"""
    H, g = normal_equations(oracle, case) if normal is None else normal
    g = g.ravel().copy()

    def bsolve(v):
        rc, d = oracle.band_solve(H, -v.reshape(-1, 15), lam)
        assert rc == 0
        return d.ravel()

    far = rw.find("far")
    if not far:
        return bsolve, g, H, None
    Ud = np.vstack([rw.J[b[3]:b[3] + b[4]] for b in far])
    U, Ut = csr_matrix(Ud), csr_matrix(np.ascontiguousarray(Ud.T))
    g += Ut @ np.concatenate([rw.r[b[3]:b[3] + b[4]] for b in far])
    Z = np.column_stack([bsolve(Ud[i]) for i in range(Ud.shape[0])])
    S = np.eye(Ud.shape[0]) + U @ Z
    Zs = csr_matrix(Z)

    def msolve(v):
        y = bsolve(v)
        return y - Zs @ np.linalg.solve(S, U @ y)
    return msolve, g, H, Ud


def restatement(oracle, case: Case, rw: Rows, lam=LAMBDA, corrections=REFINE, rel_stop=REL_STOP, A=None):
    """dict start (n, 15), x (n, 15), corrections applied, reduction (res . z at the end / at the start).  A: another
    operator (a mutation: gradient and preconditioner stay those of the case)"""
    msolve, g, _, _ = preconditioner(oracle, case, rw, lam)
    A = operator(rw, lam) if A is None else A
    x = msolve(-g)
    start = x.copy()
    nres = g + A(x)
    rz, rz0, done, p = -1.0, 0.0, 0, None
    for _ in range(corrections):
        z = msolve(-nres)
        s = float(-nres @ z)
        first = rz < 0.0
        if not (s > 0.0) or (not first and s <= rel_stop * rel_stop * rz0):
            rz = s if s > 0.0 else rz            # (the value the rule stopped at is the one of the x that stays)
            break
        p = z if first else z + (s / rz) * p
        rz = s
        if first:
            rz0 = s
        Ap = A(p)
        pAp = float(p @ Ap)
        if not (pAp > 0.0):
            break
        alpha = rz / pAp
        x = x + alpha * p
        nres = nres + alpha * Ap
        done += 1
    return dict(start=start.reshape(-1, 15), x=x.reshape(-1, 15), corrections=done, reduction=rz / rz0 if rz0 > 0.0 else 0.0)


def reference(oracle, case: Case):
    """everything the tests of one case share: rows, dref with the size of exact's last correction, the restatement"""
    rw = rows(oracle, case)
    dref, last, sizes = exact(rw, LAMBDA)
    return dict(case=case, rows=rw, dref=dref, last=last, sizes=sizes, res=restatement(oracle, case, rw))


def twin_problem(case: Case):
    """oracle/twin_qr.Problem of the window's IMU, between and X0-prior factors (window-local keyframes)"""
    from oracle import twin_qr
    c, p = case, case.prob
    sel = (p["btw_a"] >= c.lo) & (p["btw_b"] < c.hi)
    return twin_qr.Problem(c.states[c.lo:c.hi], np.arange(1, c.n), p["imu"][c.lo + 1:c.hi], p["btw_a"][sel] - c.lo, p["btw_b"][sel] - c.lo,
                           p["btw"][sel], prior_k=None if c.prior_k is None else c.prior_k - c.lo, prior_rec=None if c.prior_k is None else p["prior"])


def twin_rows(case: Case, rw: Rows) -> Rows:
    """`rw` with the residuals and Jacobians of the IMU, between and X0-prior factors evaluated by oracle/twin_qr.py instead
    of the C oracle (far factors and the marginal prior stay as they are)"""
    prob = twin_problem(case)
    lin = prob.linearize()
    J, r = rw.J.copy(), rw.r.copy()
    for kind, w in (("imu", 15), ("btw", 6)):
        if not rw.find(kind):                   # (a window of two keyframes has no between factor and the twin no "btw")
            continue
        rt, Jt = lin[kind]
        for f, (_, a, b, r0, nr) in enumerate(rw.find(kind)):
            if kind == "btw":
                assert (a, b) == (prob.btw_a[f], prob.btw_b[f])
            J[r0:r0 + nr, 15 * a:15 * a + w], J[r0:r0 + nr, 15 * b:15 * b + w] = Jt[f][:, :w], Jt[f][:, w:]
            r[r0:r0 + nr] = rt[f]
    for _, a, _, r0, nr in rw.find("prior"):
        r[r0:r0 + nr], J[r0:r0 + nr, 15 * a:15 * a + 15] = lin["prior"]
    return Rows(J, r, rw.L, rw.g_mp, rw.blocks)


def input_sensitivity(case: Case, rw: Rows, dref):
    """err(exact of the twin's rows, dref): what U_CASE records"""
    return err(exact(twin_rows(case, rw), LAMBDA)[0], dref)


def err(x, dref):
    """max |x - dref|, every tangent component divided by the largest |dref| of that component over the window"""
    x, dref = np.asarray(x).reshape(-1, 15), np.asarray(dref).reshape(-1, 15)
    return float(np.max(np.abs(x - dref) / np.max(np.abs(dref), axis=0)))


# ---------------------------------------------------------------- mutations of the operator (the bar can fail)
def _without(rw: Rows, row0, nrows, col0=None, ncols=None):
    J = rw.J.copy()
    if col0 is None:
        J[row0:row0 + nrows] = 0.0
    else:
        J[row0:row0 + nrows, col0:col0 + ncols] = 0.0
    return Rows(J, rw.r, rw.L, rw.g_mp, rw.blocks)


def mutations(case: Case, rw: Rows, lam=LAMBDA):
    """{name: operator}: the case's operator wrong in ONE row class"""
    out = {}
    span3 = [b for b in rw.find("btw") if b[2] - b[1] == 3]
    f = span3[len(span3) // 2]
    out["span-3 between factor without its a block"] = operator(_without(rw, f[3], 6, 15 * f[1], 6), lam)
    out["span-3 between factor without its rows"] = operator(_without(rw, f[3], 6), lam)
    out["no lambda"] = operator(rw, 0.0)
    if case.prior_k is not None:
        f = rw.find("prior")[0]
        out["X0 prior's rows dropped"] = operator(_without(rw, f[3], 15), lam)
    f = rw.find("imu")[-1]
    zero_bias = _without(_without(rw, f[3], 15, 15 * f[1] + 9, 6), f[3], 15, 15 * f[2] + 9, 6)
    out["bias columns of the last IMU factor dropped"] = operator(zero_bias, lam)
    if case.far is not None:
        f = rw.find("far")[-1]
        out["a block of the last far factor dropped"] = operator(_without(rw, f[3], 6, 15 * f[1], 6), lam)
    if case.marg is not None:
        L = rw.L.copy()
        L[30:36, :] = 0.0
        out["marginal prior's rows of keyframe lo + 2 dropped"] = operator(Rows(rw.J, rw.r, L, rw.g_mp, rw.blocks), lam)
    return out
