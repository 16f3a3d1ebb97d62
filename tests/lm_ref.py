"""The LM decision rule of K5 (k_decide, k_model_change, k_close_excursion, k_reset_lambda), restated as a plain state machine.

Written from the rule as include/vilfusion.h (accept_rel, lm_excursion, min_model_fidelity, vf_engine_set_convergence) and
DESIGN.md section 4a state it, not from the kernel and not around vfo_lm:

  * a trial is judged against the reference cost: the kept cost, or, while an excursion is open, the cost of the point the
    excursion left;
  * it is good iff its cost is below reference (1 + accept_rel); under GTSAM's rule (min_model_fidelity > 0) iff the decrease
    the linearised problem predicts is positive and (reference - cost) / predicted exceeds min_model_fidelity.  A trial whose
    solve failed is never good;
  * good: accepted (1), lambda / down, an open excursion ends with everything kept;
  * not good, solved, fewer than W provisional trials so far: kept provisionally (2), lambda / down^2; the first such trial
    opens the excursion and remembers the point and the cost it leaves;
  * not good otherwise: with an excursion open the point it left comes back (3), without one the trial is dropped (0); either
    way lambda * up and the trial counts as rejected;
  * lambda stays within [lambda_min, lambda_max];
  * termination (when a tolerance is set): a solved trial that ends 0 or 1 and moves the cost by <= abs_tol or <= rel_tol x
    reference, in either direction, stops the window;
  * a solve starts from lambda0 unless the damping is carried; an excursion still open at the end of a solve is undone.

Carry, as established on the MI355X (tests/test_gpu_lm_trace.py::test_damping_carries_between_solves): an engine with
lm_excursion > 0 carries the damping of EVERY window from one vf_engine_iterate to the next, whether or not the solve ended
inside an excursion; an engine with lm_excursion = 0 starts every solve from lambda0.  end_solve() pins that.

The cost bar.  S = the largest relative distance between the oracle's float64 cost and a 50-digit evaluation of the same
cost (tests/mp_lie.py's residuals) at the first three trial points of a case; measured by tests/test_lm_ref_host.py:

    S_CASE below, per case: 1e-16 .. 2e-15 at the perturbed starts (costs of 1e8 .. 1e12), 3.1e-13 at the optimum of case
    "stop" (cost 0.03)

The bar on a cost is 16 S + 64 eps (16 as elsewhere in this suite: a correct float64 evaluation in another order), and MARGIN,
the least relative distance of any committed decision from its threshold, is fixed at 1e-6: 1.6e5 x the largest bar (6.3e-12,
case "stop") and 2e7 x the bars of the other cases (5e-14).  The smallest margin any committed decision has is 0.033 (rej_acc8's first accepted trial).

Blind spots (tests/test_lm_ref_host.py prints the table):
  * "a failed solve that leaves an open excursion in place" is caught by no committed case: no window of <= 40 keyframes with a
    prior has a band solve that fails while an excursion is open.  SCRIPTED_FAIL below catches it in the machine alone (the
    host test runs it); on the device that branch is reached by no test.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from tests import helpers
from vil_sensor_fusion_amd import synth

EPS = 2.0 ** -52
ACCEPT_REL = 1e-9          # vf_engine_opts.accept_rel's default (include/vilfusion.h)
BAR_FACTOR = 16.0
MARGIN = 1e-6


@dataclass(frozen=True)
class Case:
    name: str
    seed: int
    n: int                 # keyframes loaded
    lo: int
    hi: int
    perturb: float
    lam0: float
    up: float
    down: float
    lmin: float
    lmax: float
    W: int                 # lm_excursion
    min_fidelity: float
    K: int
    rel_tol: float = 0.0   # vf_engine_set_convergence (0, 0: off)
    abs_tol: float = 0.0
    accept_rel: float = 1e-9     # vf_engine_opts.accept_rel (its default)


# (name, seed, n, lo, hi, perturb, lambda0, up, down, lmin, lmax, W, min_fidelity, K[, rel_tol, abs_tol[, accept_rel]])
CASES = tuple(Case(*c) for c in (
    ("rej_acc", 7, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 0.0, 12),
    ("rej_acc8", 8, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 0.0, 9),
    ("exc_ok", 6, 33, 0, 33, 0.6, 1e-5, 10.0, 10.0, 1e-12, 1e-2, 2, 0.0, 5),
    ("exc_ok3", 7, 33, 0, 33, 0.6, 1e-5, 10.0, 10.0, 1e-12, 1e10, 3, 0.0, 5),
    ("exc_fail", 1, 33, 0, 33, 1.0, 1e-5, 10.0, 10.0, 1e-12, 1e-2, 2, 0.0, 12),
    ("all_rej", 1, 33, 0, 33, 1.0, 1e-5, 10.0, 10.0, 1e-12, 1e-2, 0, 0.0, 12),
    # the window [3, 36) of 40 loaded keyframes; its last trial leaves an excursion open, which the end of the solve undoes
    ("range", 1, 40, 3, 36, 1.0, 1e-5, 10.0, 10.0, 1e-12, 1e10, 2, 0.0, 8),
    # GTSAM's rule.  At its own threshold (1e-3) no window of <= 33 keyframes has a trial on which the two rules disagree away
    # from the rounding floor (seeds 0 .. 11, perturbations 0.3 .. 1, lambda0 1e-5 .. 100: they part only where the predicted
    # decrease is <= 0 or the last bit decides); at 0.25 they do, by 0.2: fid25's trial 4 lowers the cost and is rejected
    ("fid", 7, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 1e-3, 8),
    ("fid25", 8, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 0.25, 8),
    ("stop", 3, 33, 0, 33, 0.05, 1e-5, 10.0, 10.0, 1e-12, 1e-2, 0, 0.0, 12, 1e-5, 1e-5),
    # a REJECTED trial within the tolerance stops the window: rej_acc's first trial raises the cost 2.38-fold, rel_tol = 2
    ("stop_rej", 7, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 0.0, 3, 2.0, 0.0),
    # accept_rel at work: MARGIN is 1000 x the default accept_rel, so no decisive trial lies between "decreases" and "decreases
    # or rises by less than accept_rel" unless accept_rel is large
    ("rel_half", 7, 33, 0, 33, 0.8, 1.0, 10.0, 10.0, 1e-12, 1e10, 0, 0.0, 8, 0.0, 0.0, 0.5),
))
BY_NAME = {c.name: c for c in CASES}

# S per case: the measurement of tests/test_lm_ref_host.py::test_cost_bar (in the comment) rounded up by a quarter; the test
# asserts that a fresh measurement is no larger and no less than a quarter of it
S_CASE = {
    "rej_acc": 2.2e-15,     # 1.75e-15
    "rej_acc8": 1.8e-15,    # 1.41e-15
    "exc_ok": 9.0e-16,      # 7.23e-16
    "exc_ok3": 2.0e-15,     # 1.62e-15
    "exc_fail": 2.5e-15,    # 2.02e-15
    "all_rej": 2.5e-15,     # 2.02e-15
    "range": 1.5e-15,       # 1.16e-15
    "fid": 2.2e-15,         # 1.75e-15
    "fid25": 1.8e-15,       # 1.41e-15
    "stop": 3.9e-13,        # 3.14e-13 (its third trial point is the optimum: cost 0.03, the sum of residuals that cancel)
    "stop_rej": 1.3e-16,    # 1.06e-16 (one trial point: the window stops at its first trial)
    "rel_half": 2.2e-15,    # 1.75e-15
}


def bar(name):
    """the bar on a relative cost difference of a case"""
    return BAR_FACTOR * S_CASE[name] + 64.0 * EPS


MUTATIONS = (
    "strict_decrease",          # strict decrease instead of accept_rel
    "prov_le_W",                # prov <= W instead of prov < W
    "prov_divides_once",        # a provisional trial divides lambda once
    "judge_against_previous",   # an excursion judged against the previous trial's cost instead of ref_cost
    "ref_cost_retaken",         # ref_cost retaken on every provisional trial
    "no_clamp_lmin",
    "no_clamp_lmax",
    "restore_keeps_lambda",     # outcome 3 does not multiply lambda by up
    "stop_on_accepted_only",    # termination applied to accepted trials only
    "failed_solve_keeps_excursion",   # a failed solve leaves an open excursion in place instead of restoring it
)


class Machine:
    """the state of one window.  `point` is whatever the caller uses to name a point of the state space (an array of states);
    the machine only keeps, saves and restores it."""

    def __init__(self, case: Case, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.p, self.accept_rel, self.mut = case, case.accept_rel, mutation
        self.cost = self.ref_cost = math.nan
        self.lam = case.lam0
        self.prov = 0
        self.point = self.saved = None
        self.acc = self.rej = self.prov_total = self.fails = 0
        self.done = False
        self.carry = False

    # ---- the thresholds
    def refc(self):
        if self.prov > 0 and self.mut != "judge_against_previous":
            return self.ref_cost
        return self.cost

    def good(self, c, solved, predicted=None):
        if not solved:
            return False
        ref = self.refc()
        if self.p.min_fidelity > 0.0:
            return predicted > 0.0 and (ref - c) > self.p.min_fidelity * predicted
        if self.mut == "strict_decrease":
            return c < ref
        return c < ref * (1.0 + self.accept_rel)

    def stops(self, c):
        dec = abs(self.refc() - c)
        return dec <= self.p.abs_tol or dec <= self.p.rel_tol * self.refc()

    # ---- a solve
    def begin_solve(self, cost, point=None):
        if not self.carry:
            self.lam = self.p.lam0
        self.carry = False
        self.cost, self.point, self.prov, self.done = cost, point, 0, False

    def step(self, c, solved, predicted=None, point=None):
        """one trial at cost c (`point`: where it is); returns the outcome"""
        p = self.p
        good = self.good(c, solved, predicted)
        room = self.prov <= p.W if self.mut == "prov_le_W" else self.prov < p.W
        if good:
            outcome = 1
        elif p.W > 0 and solved and room:
            outcome = 2
        elif self.prov > 0 and not (self.mut == "failed_solve_keeps_excursion" and not solved):
            outcome = 3
        else:
            outcome = 0
        if not solved:
            self.fails += 1
        if (p.rel_tol > 0.0 or p.abs_tol > 0.0) and solved and (outcome == 1 if self.mut == "stop_on_accepted_only" else outcome < 2):
            if self.stops(c):
                self.done = True
        if outcome in (1, 2):
            if outcome == 2 and (self.prov == 0 or self.mut == "ref_cost_retaken"):
                self.ref_cost = self.cost
                if self.prov == 0:
                    self.saved = self.point
            self.cost, self.point = c, point
            if outcome == 1:
                self.acc += 1
                self.prov = 0
                self.lam = self.lam / p.down
            else:
                self.prov_total += 1
                self.prov += 1
                self.lam = self.lam / (p.down if self.mut == "prov_divides_once" else p.down * p.down)
            if self.mut != "no_clamp_lmin":
                self.lam = max(self.lam, p.lmin)
        else:
            self.rej += 1
            if outcome == 3:
                self.cost, self.point, self.prov = self.ref_cost, self.saved, 0
            if not (outcome == 3 and self.mut == "restore_keeps_lambda"):
                self.lam = self.lam * p.up
            if self.mut != "no_clamp_lmax":
                self.lam = min(self.lam, p.lmax)
        return outcome

    def end_solve(self):
        """the end of a vf_engine_iterate: an open excursion is undone; an engine that runs excursions carries its damping.
        Returns whether a point was restored."""
        restored = self.prov > 0
        if restored:
            self.cost, self.point, self.prov = self.ref_cost, self.saved, 0
        self.carry = self.p.W > 0
        return restored

    def counters(self):
        return (self.acc, self.rej, self.prov_total, self.fails)


def accept_margin(m: Machine, c, solved=True, predicted=None):
    """relative distance of the accept decision from its threshold (inf for a failed solve: nothing is compared)"""
    if not solved:
        return math.inf
    ref = m.refc()
    if m.p.min_fidelity > 0.0:
        if not predicted > 0.0:
            return abs(predicted) / ref
        return abs((ref - c) / predicted - m.p.min_fidelity)
    return abs(c - ref * (1.0 + m.accept_rel)) / ref


def stop_margin(m: Machine, c, solved=True):
    """... of the termination rule: the nearer of its two tolerances (inf when the rule is off)"""
    if not solved or not (m.p.rel_tol > 0.0 or m.p.abs_tol > 0.0):
        return math.inf
    dec, out = abs(m.refc() - c), math.inf
    if m.p.abs_tol > 0.0:
        out = min(out, abs(dec - m.p.abs_tol) / m.p.abs_tol)
    if m.p.rel_tol > 0.0:
        tol = m.p.rel_tol * m.refc()
        out = min(out, abs(dec - tol) / tol)
    return out


def margin(c, m: Machine, solved=True, predicted=None):
    """the least relative distance of what step(c, ...) is about to decide from a threshold.  Call BEFORE step."""
    return min(accept_margin(m, c, solved, predicted), stop_margin(m, c, solved))


# ---------------------------------------------------------------- problems and the oracle as evaluator
_problems = {}


def problem(oracle, case: Case):
    key = (case.seed, case.n, case.perturb)
    if key not in _problems:
        _problems[key] = helpers.build_problem(oracle, synth.make_sequence(case.seed, case.n), case.perturb)
    return _problems[key]


def window_at(oracle, prob, states, lo, hi):
    """the oracle's Window over [lo, hi) with `states` (all loaded keyframes) in place of the problem's"""
    return helpers.oracle_window(oracle, dict(prob, states=np.asarray(states)), lo, hi)


def retract_all(oracle, states, delta):
    return np.array([oracle.retract(s, d) for s, d in zip(states, delta)])


def predicted_decrease(oracle, prob, states, lo, hi, delta):
    """0.5 |r|^2 - 0.5 |r + J d|^2 over the oracle's whitened rows at `states` (all loaded keyframes), d: (hi - lo, 15)"""
    from tests import refine_ref as rr
    rw = rr.rows(oracle, rr.Case("lm", prob, np.asarray(states), lo, hi, lo))
    lin = rw.r + rw.J @ np.asarray(delta).reshape(-1)
    return 0.5 * float(rw.r @ rw.r) - 0.5 * float(lin @ lin)


def mp_cost(prob, states, lo, hi):
    """the window's cost 0.5 sum |r|^2 at 50 digits (tests/mp_lie.py's residuals); returns an mpf"""
    from tests import mp_lie as ml
    st = [ml.State.of(s) for s in states]
    g = ml.vec(prob["gravity"])
    total = ml.mp.mpf(0)
    for k in range(lo + 1, hi):
        total += sum(x * x for x in ml.imu_residual(prob["imu"][k], g, st[k - 1], st[k]))
    for a, b, rec in zip(prob["btw_a"], prob["btw_b"], prob["btw"]):
        if a >= lo and b < hi:
            total += sum(x * x for x in ml.between_residual(rec, st[a], st[b]))
    total += sum(x * x for x in ml.prior_residual(prob["prior"], st[lo]))
    return total / 2


# ---------------------------------------------------------------- the driver on the oracle
@dataclass
class Trace:
    outcomes: list = field(default_factory=list)     # per trial; -1: not run (the window had stopped)
    lam_used: list = field(default_factory=list)     # the damping a trial ran with
    lam: list = field(default_factory=list)          # ... and the damping after it
    cost: list = field(default_factory=list)         # kept cost after the trial
    trial_cost: list = field(default_factory=list)   # the trial's own cost
    prov: list = field(default_factory=list)
    accept_margin: list = field(default_factory=list)
    stop_margin: list = field(default_factory=list)
    done: list = field(default_factory=list)
    rule_differs: list = field(default_factory=list)   # fidelity cases: the accept_rel rule would have decided otherwise
    trial_points: list = field(default_factory=list)
    counters: tuple = ()
    final_cost: float = math.nan
    final_lam: float = math.nan
    closed: bool = False
    cost0: float = math.nan
    final_point: np.ndarray | None = None

    def key(self):
        """what two traces are compared by"""
        return (tuple(self.outcomes), tuple(self.lam), self.final_lam, self.closed)

    def string(self):
        return "".join("-" if o < 0 else str(o) for o in self.outcomes)


def run_host(oracle, case: Case, mutation=None, fail_at=(), solves=None) -> Trace:
    """the machine on the oracle's Window: assemble, oracle.band_solve, retract, cost.  fail_at: trials whose solve is
    declared failed (SCRIPTED_FAIL only).  solves: trials per vf_engine_iterate, one after the other on the same window
    (default: one solve of case.K trials); the trace runs on through them."""
    prob = problem(oracle, case)
    lo, hi = case.lo, case.hi
    states = prob["states"].copy()
    m = Machine(case, mutation=mutation)
    tr = Trace()
    cost, H, g = window_at(oracle, prob, states, lo, hi).assemble()
    tr.cost0 = cost
    m.begin_solve(cost, states)
    ends = list(np.cumsum(solves if solves is not None else (case.K,)))
    for t in range(ends[-1]):
        if t in ends:
            m.end_solve()
            _, H, g = window_at(oracle, prob, m.point, lo, hi).assemble()
            m.begin_solve(m.cost, m.point)
        if m.done:
            tr.trial_cost.append(math.nan)
            tr.outcomes.append(-1); tr.lam_used.append(m.lam); tr.lam.append(m.lam); tr.cost.append(m.cost); tr.prov.append(m.prov)
            tr.accept_margin.append(math.inf); tr.stop_margin.append(math.inf); tr.done.append(True); tr.rule_differs.append(False)
            continue
        rc, d = oracle.band_solve(H, g, m.lam)
        solved = rc == 0 and t not in fail_at
        c, predicted, trial, Ht, gt = math.nan, None, None, None, None
        if solved:
            trial = m.point.copy()
            trial[lo:hi] = retract_all(oracle, m.point[lo:hi], d)
            c, Ht, gt = window_at(oracle, prob, trial, lo, hi).assemble()
            if case.min_fidelity > 0.0:
                predicted = predicted_decrease(oracle, prob, m.point, lo, hi, d)
            if len(tr.trial_points) < 3:
                tr.trial_points.append((trial, c))
        tr.lam_used.append(m.lam)
        tr.trial_cost.append(c)
        tr.accept_margin.append(accept_margin(m, c, solved, predicted))
        tr.stop_margin.append(stop_margin(m, c, solved))
        tr.rule_differs.append(bool(solved and case.min_fidelity > 0.0 and
                                    (c < m.refc() * (1.0 + m.accept_rel)) != m.good(c, solved, predicted)))
        out = m.step(c, solved, predicted, trial)
        if out in (1, 2):
            H, g = Ht, gt
        elif out == 3:
            _, H, g = window_at(oracle, prob, m.point, lo, hi).assemble()
        tr.outcomes.append(out); tr.lam.append(m.lam); tr.cost.append(m.cost); tr.prov.append(m.prov); tr.done.append(m.done)
    tr.closed = m.end_solve()
    tr.counters, tr.final_cost, tr.final_lam = m.counters(), m.cost, m.lam
    tr.final_point = m.point
    return tr


def run_vfo(oracle, case: Case):
    """vfo_lm on the same window: (costs K + 1, outcomes K, final lambda, states)"""
    prob = problem(oracle, case)
    win = helpers.oracle_window(oracle, prob, case.lo, case.hi)
    costs, acc, lam = win.lm(iterations=case.K, lambda0=case.lam0, up=case.up, down=case.down, lmin=case.lmin, lmax=case.lmax,
                             rel_tol=case.rel_tol, abs_tol=case.abs_tol, accept_rel=case.accept_rel, excursion=case.W, min_model_fidelity=case.min_fidelity)
    return costs, [int(a) for a in acc], lam, win.states


# "a failed solve that leaves an open excursion in place": the machine alone, on case exc_ok with the solve of trial 1 (the
# second provisional trial) declared failed -- the rule restores the point the excursion left (3); the mutation drops the trial (0)
SCRIPTED_FAIL = ("exc_ok", (1,))
BLIND_SPOTS = ("failed_solve_keeps_excursion",)      # mutations that no committed case catches
