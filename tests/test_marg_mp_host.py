"""CPU: the extended-precision reference of the fixed-lag marginalisation (tests/mp_marg.py) and its derived bound, proved on
the host before any device run: a plain float64 twin and the C oracle's Window.marginalize stay within c 2^-53 B on every case
of tests/marg_cases.py (linearisations from the oracle), and six seeded mutations of the twin each leave it."""
import numpy as np
import pytest

from tests import marg_cases as mc
from tests import mp_marg
from tests import mp_lie as ml


def marg_delta_f64(marg, states):
    """marg_delta (k2b_priors.inc) in float64, written out plainly: quaternion product, Log, J_l^-1 on the translation"""
    d = np.zeros(27)
    for j in range(3):
        xb, x = np.asarray(marg["xbar"][j]), np.asarray(states[j])
        qb, q = xb[0:4] / np.linalg.norm(xb[0:4]), x[0:4] / np.linalg.norm(x[0:4])
        w0, v0 = qb[0], -qb[1:4]
        qw = w0 * q[0] - v0 @ q[1:4]
        qv = w0 * q[1:4] + q[0] * v0 + np.cross(v0, q[1:4])
        if qw < 0.0:
            qw, qv = -qw, -qv
        nv = np.linalg.norm(qv)
        w = qv * (2.0 * np.arctan2(nv, qw) / nv) if nv > 0.0 else np.zeros(3)
        Rb = np.array([[1 - 2 * (qb[2] ** 2 + qb[3] ** 2), 2 * (qb[1] * qb[2] - qb[0] * qb[3]), 2 * (qb[1] * qb[3] + qb[0] * qb[2])],
                       [2 * (qb[1] * qb[2] + qb[0] * qb[3]), 1 - 2 * (qb[1] ** 2 + qb[3] ** 2), 2 * (qb[2] * qb[3] - qb[0] * qb[1])],
                       [2 * (qb[1] * qb[3] - qb[0] * qb[2]), 2 * (qb[2] * qb[3] + qb[0] * qb[1]), 1 - 2 * (qb[1] ** 2 + qb[2] ** 2)]])
        t = Rb.T @ (x[4:7] - xb[4:7])
        th2 = w @ w
        th = np.sqrt(th2)
        E = 1.0 / 12 + th2 / 720 + th2 * th2 / 30240 if th < 0.1 else 1.0 / th2 - 1.0 / (2.0 * th * np.tan(th / 2))
        u = t - 0.5 * np.cross(w, t) + E * np.cross(w, np.cross(w, t))
        o = 0 if j == 0 else 15 + 6 * (j - 1)
        d[o:o + 3], d[o + 3:o + 6] = w, u
        if j == 0:
            d[6:15] = x[7:16] - xb[7:16]
    return d


# ---------------------------------------------------------------- the twin: form the 42 x 42, eliminate 15 pivots, symmetrise
def twin(case, mut=None, lower_only=False):
    """float64, plain loops in the obvious order (not the kernel's).  mut: one of MUTATIONS.  lower_only: the pivots update
    the lower triangle and the right-hand side only (an asymmetric update) and the symmetrisation mirrors it up."""
    A = [[0.0] * 42 for _ in range(42)]
    b = [0.0] * 42
    r, J = np.array(case.imu[0]), np.array(case.imu[1])
    if mut == "jacobian_1e-9":
        kept = [mp_marg.IMU_COL[i] for i in range(15, 30)]
        r0, c0 = max(((abs(J[r_, c_]), r_, c_) for r_ in range(15) for c_ in kept))[1:]
        J[r0, c0] *= 1.0 + 1e-9
    for i in range(30):
        for j in range(30):
            s = 0.0
            for k in range(15):
                s += J[k, mp_marg.IMU_COL[i]] * J[k, mp_marg.IMU_COL[j]]
            A[i][j] += s
        s = 0.0
        for k in range(15):
            s += J[k, mp_marg.IMU_COL[i]] * r[k]
        b[i] += s
    for f in case.btw:
        ob = mp_marg.OFF[f["d"]]
        if mut == "jb_at_m+1" and f["d"] == 2:
            ob = 15
        Jf = np.hstack([f["Ja"], f["Jb"]])
        cols = list(range(6)) + list(range(ob, ob + 6))
        for a, ia in enumerate(cols):
            for c, ic in enumerate(cols):
                s = 0.0
                for k in range(6):
                    s += Jf[k, a] * Jf[k, c]
                A[ia][ic] += s
            s = 0.0
            for k in range(6):
                s += Jf[k, a] * f["r"][k]
            b[ia] += -s if mut == "eta_sign_between" else s
    if case.prior is not None:
        Jp, rp = case.prior["J"], case.prior["r"]
        for i in range(15):
            for j in range(15):
                s = 0.0
                for k in range(15):
                    s += Jp[k, i] * Jp[k, j]
                A[i][j] += s
            s = 0.0
            for k in range(15):
                s += Jp[k, i] * rp[k]
            b[i] += s
    if case.marg is not None:
        d = marg_delta_f64(case.marg, case.states)
        L, eta = case.marg["L"], case.marg["eta"]
        for i in range(27):
            g = 0.0
            for j in range(27):
                g += L[i, j] * d[j]
                A[mp_marg.MAP27[i]][mp_marg.MAP27[j]] += L[i, j]
            b[mp_marg.MAP27[i]] += g + eta[i]
    for c in range(15):
        piv = A[c][c]
        assert piv > 0.0
        for i in range(c + 1, 42):
            l = A[i][c] / piv
            for j in range(c + 1, (i + 1) if (lower_only or mut == "stale_upper") else 42):
                A[i][j] -= l * A[c][j] if not (lower_only or mut == "stale_upper") else l * A[j][c]
            if not (mut == "rhs_pivot_skipped" and c == 7):
                b[i] -= l * b[c]
    S = np.array([[A[15 + i][15 + j] for j in range(27)] for i in range(27)])
    eta = np.array(b[15:])
    if mut == "stale_upper":
        pass                                              # the symmetrisation dropped: the upper triangle is stale
    elif lower_only:
        S = np.tril(S) + np.tril(S, -1).T
    else:
        S = 0.5 * (S + S.T)
    if mut == "swap_m+2_m+3":
        p = list(range(15)) + list(range(21, 27)) + list(range(15, 21))
        S, eta = S[np.ix_(p, p)], eta[p]
    return S, eta


MUTATIONS = ["swap_m+2_m+3", "jb_at_m+1", "eta_sign_between", "stale_upper", "jacobian_1e-9", "rhs_pivot_skipped"]


# ---------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def cases(oracle):
    prob = mc.base_problem(oracle)
    out = []

    def add(name, st, lo, factors, prior_rec=None, marg=None, n_kf=4, floor_p=0.0):
        case = mc.host_case(oracle, name, st, prob["imu"][lo + 1], factors, prior_rec, marg, n_kf)
        got = mc.oracle_marginalize(oracle, st, prob["imu"][lo + 1], factors, prior_rec, marg, floor_p)
        out.append(dict(case=case, ref=mp_marg.reference(case), oracle=got, floor_p=floor_p))
        return got

    for i, sub in enumerate(mc.SUBSETS):                  # span patterns, anchor prior, 0.01 off its mean
        lo, n, st, factors, prior_rec = mc.span_inputs(oracle, prob, i)
        add(f"spans{sub}", st, lo, factors, prior_rec, n_kf=n)
    for scale in mc.CHAIN_SCALES:                         # anchor prior, then three rounds with the previous marginal prior, d != 0
        lo, st, factors = mc.chain_inputs(oracle, prob, scale, 0)
        # (the floor is requested, as the engine does by default: with the reference sigmas it must not engage)
        got = add(f"anchor-{scale}", st, lo, factors, mc.reference_prior(prob["states"][lo]), n_kf=mc.CHAIN_N,
                  floor_p=oracle.prior_gauge_floor(mc.CHAIN_N))
        for k in range(1, 4):
            lo, st, factors = mc.chain_inputs(oracle, prob, scale, k)
            marg = dict(L=got["L"], eta=got["eta"], xbar=got["xbar"])
            got = add(f"chain-{scale}-round{k}", st, lo, factors, None, marg)
    lo, n, st, factors, prior_rec = mc.weak_inputs(oracle, prob)         # weak anchor prior: the gauge floor engages at once
    add("weak-prior-floor", st, lo, factors, prior_rec, n_kf=n, floor_p=oracle.prior_gauge_floor(n))
    # inputs the reference cannot read from the code under test: the anchor prior's rows and a far factor ending at m+2 (absorbed
    # like a band factor) come from mp_lie, their rounding counted as input uncertainty; the oracle works from its own float64 rows
    lo, n, st, factors, prior_rec = mc.span_inputs(oracle, prob, 5)
    rec = mc.between_record(prob["gt"], lo, lo + 2, np.random.default_rng(22), 1e-4)
    case = mc.host_case(oracle, "rounded-prior-and-far-rows", st, prob["imu"][lo + 1], factors, None, None, n)
    rp, Jp = ml.prior_factor(prior_rec, st[0])
    case.prior = dict(r=rp, J=Jp, sig=prior_rec[16:31], rounded=True)
    rb, Ja, Jb = ml.between_factor(rec, st[0], st[2])
    case.btw.append(dict(d=2, r=rb, Ja=Ja, Jb=Jb, rounded=True, R=ml.to_np(ml.upper(ml.vec(rec[7:28]), 6))))
    got = mc.oracle_marginalize(oracle, st, prob["imu"][lo + 1], factors + [(2, rec)], prior_rec)
    out.append(dict(case=case, ref=mp_marg.reference(case), oracle=got, floor_p=0.0, twin=False))
    return out


def test_twin_and_oracle_stay_within_the_bound(cases, oracle):
    worst = {"twin": 0.0, "twin (lower triangle, mirrored)": 0.0, "oracle": 0.0}
    for e in cases:
        case, ref = e["case"], e["ref"]
        for who, lower in (("twin", False), ("twin (lower triangle, mirrored)", True)):
            if not e.get("twin", True):       # (rows taken from mpmath: a twin of them would test nothing)
                continue
            L, eta = twin(case, lower_only=lower)
            rl, re_ = mp_marg.check(case.name, L, eta, ref, what=f"{who} ")
            worst[who] = max(worst[who], rl, re_)
            assert rl <= 1.0 and re_ <= 1.0, (who, case.name, rl, re_)
        lift = ext = None
        if e["floor_p"] > 0.0:
            Q = mp_marg.gauge_basis(case.states[1:4], case.gravity)
            lift, ext, ev, _ = mp_marg.floor_lift(ref, Q, e["floor_p"])
            if case.name == "weak-prior-floor":
                assert lift is not None and min(ev) < e["floor_p"], "the case is meant to engage the floor"
                evL, slack, lv = mp_marg.floor_properties(e["oracle"]["L"], ref, Q, ext, e["floor_p"], np.random.default_rng(5))
                print(f"oracle {case.name}: eigenvalues of Q^T L Q {[float(x) for x in evL]}, floor_p {e['floor_p']:.3e}, admissible "
                      f"shortfall {float(slack):.3e}; worst |L v - S v| / bound off the gauge directions {lv:.3e}")
                assert all(x >= e["floor_p"] - slack for x in evL) and lv <= 1.0
            else:
                assert lift is None and ext is None, "reference sigmas: no admissible M reaches the floor"
        rl, re_ = mp_marg.check(case.name, e["oracle"]["L"], e["oracle"]["eta"], ref, what="oracle ", lift=lift, ext=ext)
        worst["oracle"] = max(worst["oracle"], rl, re_)
        assert rl <= 1.0 and re_ <= 1.0, ("oracle", case.name, rl, re_)
        np.testing.assert_array_equal(e["oracle"]["xbar"], case.states[1:4])
    print("worst |err| / (c 2^-53 B) over all cases:", ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutations_of_the_twin_leave_the_bound(cases, mut):
    caught = []
    for e in cases:
        case, ref = e["case"], e["ref"]
        if not e.get("twin", True):
            continue
        L, eta = twin(case, mut)
        rl, _ = mp_marg.worst_ratio(L, ref["S"], ref["B"], ref["c"])
        re_, _ = mp_marg.worst_ratio(eta, ref["eta"], ref["Beta"], ref["c"])
        if max(rl, re_) > 1.0:
            caught.append((case.name, max(rl, re_)))
    print(f"mutation {mut}: outside the bound on {len(caught)} of {len(cases)} cases; smallest excess "
          f"{min((r for _, r in caught), default=0.0):.3e}: {[n for n, _ in caught]}")
    assert caught, f"mutation {mut} stays within the bound on every case: a case is missing"


def test_structural_zeros_are_exact(cases):
    """without a span-2 factor or a previous marginal prior nothing touches the pose of m+2: B is 0 there and so is the result"""
    e = next(e for e in cases if e["case"].name == "spans(1,)")
    B = e["ref"]["B"]
    assert all(B[i][j] == 0 for i in range(15, 27) for j in range(27))
    L, _ = twin(e["case"])
    assert np.all(L[15:27] == 0.0) and np.all(e["oracle"]["L"][15:27] == 0.0)
