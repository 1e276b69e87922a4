"""hlaAssocSurv on the host: the restatement of DESIGN.md section 31 (tests/assocsurv_reference.py) against the closed forms
of the six-subject example, against the log-rank statistic and against an independent scipy.optimize maximum of a directly
written O(n^2) risk-set likelihood; Efron and Breslow without ties, a shifted covariate, the columns that cannot be fitted,
maxit; hlaAssocSurv's own host side (condition, show_hr, the likelihood-ratio test, the base table, every ValueError) driven
by the restatement in place of the device; and the safety condition of the device tests."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_reference as AR  # noqa: E402
import assocsurv_reference as S  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assoc, assocsurv  # noqa: E402

EST_BOUND, SE_BOUND = 1e-5, 5e-3           # against an exact maximum: Newton's stopping error and the se rule of item 6


def _gap(got_est, got_se, want_est, want_se):
    return abs(got_est - want_est) / max(abs(want_est), want_se), abs(got_se / want_se - 1.0)


# 1 closed forms --------------------------------------------------------------------------------------------------
def _six(ties, epsilon=1e-12):
    time, status, x = np.array([1, 1, 6, 6, 8, 9.0]), np.array([1, 0, 1, 1, 0, 1]), np.array([1, 1, 1, 0, 0, 0.0])
    o = np.argsort(-time, kind="stable")
    return S.fit(x[o][:, None], status[o], S.Blocks(time[o]), [0.0], 1, ties, 20, epsilon)


def test_six_subject_example():
    """time (1,1,6,6,8,9), status (1,0,1,1,0,1), x (1,1,1,0,0,0): Breslow's estimate is log((3 + sqrt 33) / 2), Efron's log r
    with r the positive root of 2 - r/(r+1) - r/(r+3) - r/(r+5) = 0."""
    r = _six("breslow")
    assert r["flags"] == 0 and abs(r["coef"][0] - math.log((3 + math.sqrt(33)) / 2)) <= 1e-9

    def g(v):
        return 2 - v / (v + 1) - v / (v + 3) - v / (v + 5)

    lo, hi = 1.0, 100.0
    assert g(lo) > 0 > g(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) > 0 else (lo, mid)
    r = _six("efron")
    assert r["flags"] == 0 and abs(r["coef"][0] - math.log(0.5 * (lo + hi))) <= 1e-9
    assert np.isfinite(r["se"][0]) and r["loglik"] < 0 and r["score"] > 0


def test_efron_and_breslow_agree_without_ties():
    c = S.device_cohort("n40")
    assert S.Blocks(c["time"]).nb == len(c["time"])
    a, b = S.reference("n40", "dominant", "efron"), S.reference("n40", "dominant", "breslow")
    for key in ("coef", "se", "loglik", "score", "iterations", "flags"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    a, b = S.reference("n255", "dominant", "efron"), S.reference("n255", "dominant", "breslow")
    assert not np.allclose(a["coef"][1:, 0], b["coef"][1:, 0], rtol=1e-6, equal_nan=True)      # (with ties they differ)


def _log_rank(time, event, x):
    """The textbook statistic: (O - E)^2 / V over the distinct event times, V the hypergeometric variance."""
    o_e = var = 0.0
    for t in np.unique(time[event == 1]):
        at_risk, died = time >= t, (time == t) & (event == 1)
        n, n1, d, d1 = at_risk.sum(), (at_risk & (x == 1)).sum(), died.sum(), (died & (x == 1)).sum()
        o_e += d1 - d * n1 / n
        if n > 1:
            var += d * (n1 / n) * (1 - n1 / n) * (n - d) / (n - 1)
    return o_e * o_e / var


def test_score_statistic_is_the_log_rank_test():
    """One binary column, no covariates, no ties: score_stat = the log-rank statistic.  (With ties Breslow's information is
    the hypergeometric variance times (n - 1) / (n - d) per event time, so only the tie-free case is the textbook test.)"""
    c = S.device_cohort("n40")
    A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, "dominant")
    r = S.reference("n40", "dominant")
    seen = 0
    for t in range(A.n_tests):
        if r["flags"][1 + t] & S.RANK_BIT:
            continue
        want = _log_rank(c["time"], A.y, A.F[t])
        assert abs(r["score"][1 + t] - want) <= 1e-10 * max(want, 1.0), (t, r["score"][1 + t], want)
        seen += 1
    assert seen >= 4
    assert abs(_six("breslow")["score"] - 1.6) <= 1e-12


# 2 an independent maximum of the likelihood ----------------------------------------------------------------------
def _mle(X, time, event, ties):
    """The maximum of the partial likelihood written over explicit risk sets, one row per distinct event time."""
    optimize = pytest.importorskip("scipy.optimize")
    times = np.unique(time[event == 1])
    R = (time[None, :] >= times[:, None]).astype(float)                       # [K, n]: at risk
    D = ((time[None, :] == times[:, None]) & (event[None, :] == 1)).astype(float)
    d = D.sum(axis=1).astype(int)
    kk = np.repeat(np.arange(len(times)), d)
    f = np.concatenate([np.arange(v) / v for v in d]) if ties == "efron" else np.zeros(len(kk))
    Wm = R[kk] - f[:, None] * D[kk]                                           # [events, n]: the weight of r_j in phi_kl
    ev = event == 1

    def parts(b):
        r = np.exp(X @ b)
        phi = Wm @ r
        num = Wm @ (r[:, None] * X)
        return r, phi, num

    def nll(b):
        return float(np.log(parts(b)[1]).sum() - (X[ev] @ b).sum())

    def grad(b):
        r, phi, num = parts(b)
        return (num / phi[:, None]).sum(axis=0) - X[ev].sum(axis=0)

    def hess(b):
        r, phi, num = parts(b)
        v = num / phi[:, None]
        w = (Wm / phi[:, None]).sum(axis=0) * r
        return X.T @ (X * w[:, None]) - v.T @ v

    b = optimize.minimize(nll, np.zeros(X.shape[1]), jac=grad, hess=hess, method="trust-exact", options={"gtol": 1e-12}).x
    for _ in range(3):                                          # Newton steps at the optimum: the gradient down to rounding
        b = b - np.linalg.solve(hess(b), grad(b))
    assert np.linalg.norm(grad(b)) <= 1e-10
    return b, np.sqrt(np.diag(np.linalg.inv(hess(b))))


# (samples, alleles, covariates, seed, distinct times or None, ties rule): five common alleles, so that every genotype class
# of every allele has events and non-events -- a column whose carriers have no event has no finite maximum to compare with
MLE_COHORTS = [(300, 5, 0, 21, None, "efron"), (300, 5, 2, 22, 10, "efron"), (301, 5, 5, 23, 10, "breslow"), (299, 5, 3, 24, 25, "efron")]


@pytest.mark.parametrize("model", S.MODELS)
def test_against_an_independent_mle(model):
    """Fits with bit 0 or 2 in the restatement are left out and counted: at most a quarter (with these seeds: none).
    Measured over the four models: est within 1.0e-07 in units of max(|est|, se), se within 2.4e-04 relative."""
    worst = [0.0, 0.0]
    seen = left_out = 0
    for n, n_allele, q, seed, distinct, ties in MLE_COHORTS:
        a1, a2, time, event, _, covar = S.cohort(n, n_allele, q, seed, False, distinct)
        A, time, covar = S.analysis(a1, a2, time, event, n_allele, None, model, covar)
        r = S.cox_rows(A.F, model, time, covar, A.y, ties)
        slots = [(-1, -1)] + S.fit_slots(A.rsum, model, A.n)
        for f, rows in enumerate(slots):
            if rows is None or r["flags"][f] & S.RANK_BIT or (f == 0 and q == 0):
                continue
            if r["flags"][f] & (S.MAXIT_BIT | S.CLAMP_BIT):
                left_out += 1
                continue
            used = [i for i, row in enumerate(rows) if row >= 0] + list(range(S.COV0, S.COV0 + q))
            X = np.stack([A.F[row].astype(float) for row in rows if row >= 0] + list(covar), axis=1)
            b, se = _mle(X, time, A.y, ties)
            for j, slot in enumerate(used):
                ge, gs = _gap(r["coef"][f, slot], r["se"][f, slot], b[j], se[j])
                worst = [max(worst[0], ge), max(worst[1], gs)]
                assert ge <= EST_BOUND and gs <= SE_BOUND, (n, model, f, slot, ge, gs)
            seen += 1
    assert seen >= 15 and 4 * left_out <= seen + left_out, (seen, left_out)
    print(f"{model}: est {worst[0]:.3g}, se {worst[1]:.3g} over {seen} fits, {left_out} fits left out")


# 3 invariance, columns that cannot be fitted, maxit ---------------------------------------------------------------
def test_shifting_a_covariate_changes_nothing_but_rounding():
    hla, time, event, groups, covar = S.hla_of("n256")
    a = hb.hlaAssocSurv(hla, time, event, covar, _backend=S.Backend)
    shifted = covar.copy()
    shifted[:, 1] += 1000.0
    b = hb.hlaAssocSurv(hla, time, event, shifted, _backend=S.Backend)
    assert np.array_equal(a.flags, b.flags) and np.array_equal(a.iterations, b.iterations)
    for key in ("est", "se", "loglik", "score_stat"):
        assert np.allclose(getattr(a, key), getattr(b, key), rtol=1e-9, atol=0, equal_nan=True), key
    assert np.allclose(a.base["est"], b.base["est"], rtol=1e-9, atol=0)


def test_unfittable_columns():
    n = 30
    rng = np.random.default_rng(4)
    time = np.sort(rng.exponential(1.0, n))[::-1].copy()
    e = rng.integers(0, 2, n)
    e[:4] = 1
    zero, one, two = np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2, np.int64)
    some = (np.arange(n) % 3 == 0).astype(np.int64)
    few = (np.arange(n) % 7 == 1).astype(np.int64)
    for model, F, want in (("dominant", np.stack([zero, one, some]), [2, 2, 0]),
                           ("recessive", np.stack([zero, one, some]), [2, 2, 0]),
                           ("additive", np.stack([zero, two, one, some + few]), [2, 2, 2, 0])):     # all het: the pivot rule
        r = S.cox_rows(F, model, time, None, e)
        assert r["flags"][0] == 0 and r["iterations"][0] == 0 and np.isfinite(r["loglik"][0])       # the base model: beta = 0
        assert (r["flags"][1:] & 3).tolist() == want, model
        for t, fl in enumerate(want):
            assert np.isnan(r["coef"][1 + t]).all() == (fl == 2) and np.isnan(r["loglik"][1 + t]) == (fl == 2)
    # genotype: rows (het, hom) per test -- both empty; nobody without; no hom; no het; both
    F = np.stack([zero, zero, some, 1 - some, some, zero, zero, few, some, few])
    r = S.cox_rows(F, "genotype", time, None, e)
    assert (r["flags"][1:] & 2).tolist() == [2, 2, 0, 0, 0]
    fitted = np.isfinite(r["coef"][1:, 0:2])
    assert fitted.tolist() == [[False, False], [False, False], [True, False], [False, True], [True, True]]
    assert np.array_equal(np.isfinite(r["se"][1:, 0:2]), fitted)
    alone = S.cox_rows(some[None, :], "dominant", time, None, e)                # the one fitted dummy is that row's own fit
    assert r["coef"][3, 0] == alone["coef"][1, 0] and r["se"][3, 0] == alone["se"][1, 0] and r["score"][3] == alone["score"][1]
    # a covariate equal to a test's column: the pivot rule
    cov = S.centred(some[None, :].astype(float))
    r = S.cox_rows(np.stack([some, few]), "dominant", time, cov, e)
    assert (r["flags"] & 2).tolist() == [0, 2, 0]
    # no event: nothing is fitted
    r = S.cox_rows(np.stack([some, few]), "dominant", time, cov, np.zeros(n, int))
    assert (r["flags"] == 2).all() and np.isnan(r["loglik"]).all()
    # carriers without an event: a monotone likelihood, fitted as it comes -- every step moves the estimate by about -1 and
    # halves the gain, so it runs into maxit (bit 0) or, with enough iterations, stops where the gain is within epsilon
    lucky = np.zeros(n, np.int64)
    lucky[np.flatnonzero(e == 0)[:3]] = 1
    for maxit, want in ((10, S.MAXIT_BIT), (40, 0)):
        r = S.cox_rows(lucky[None, :], "dominant", time, None, e, maxit=maxit)
        assert r["flags"][1] == want and r["iterations"][1] == (10 if want else r["iterations"][1]) > 9
        assert r["coef"][1, 0] < -8 and r["se"][1, 0] > 30 and r["loglik"][1] > r["loglik"][0] and np.isfinite(r["score"][1])


def test_maxit_2_sets_bit_0():
    for model in S.MODELS:
        r = S.reference("n257", model, maxit=2)
        fitted = (r["flags"] & S.RANK_BIT) == 0
        assert fitted.sum() >= 4 and ((r["flags"][fitted] & S.MAXIT_BIT) != 0).sum() >= fitted.sum() - 1
        assert (r["iterations"][fitted] <= 2).all() and np.isfinite(r["loglik"][fitted]).all()
        full = S.reference("n257", model)
        assert (full["loglik"][fitted] >= r["loglik"][fitted] - 1e-9).all()


# 4 the safety condition of the device tests ----------------------------------------------------------------------
@pytest.mark.parametrize("run", S.DEVICE_RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_no_criterion_near_epsilon(run):
    """No convergence criterion of any compared fit lies within 1e-6 (relative) of epsilon, so that a device whose sums
    differ in the last bits takes the same number of iterations; and the tolerance of the device tests exists.  Of THESE runs
    only the single-event case meets a monotone likelihood that runs into maxit, so only there is the tolerance large; the
    cohorts of tests/assoc_hard_corpus.py meet monotone likelihoods in every run (carriers without an event, carriers with the
    longest follow-ups, a covariate that orders the samples as their times do), and tests/test_assoc_hard_host.py asserts this
    condition for them."""
    r = S.reference(*run)
    for f, crits in enumerate(r["crit"]):
        for c in crits:
            assert abs(c - 1e-9) > 1e-6 * 1e-9, (run, f, c)
    assert 1e-12 <= S.tolerance(*run) <= (1e-3 if run[0] == "one_event" else 1e-6), S.tolerance(*run)


def _top_hit(case="n1000"):
    hla, time, event, groups, covar = S.hla_of(case)
    res = hb.hlaAssocSurv(hla, time, event, covar, groups=groups, _backend=S.Backend)
    return hla, time, event, groups, covar, res, res.name[int(np.nanargmin(res.pval[:, 0]))]


def test_no_criterion_near_epsilon_end_to_end():
    """The same for the end-to-end runs of the device tests: n1000 dominant, plain and conditioned on its top hit, and n257
    genotype under Breslow's rule."""
    hla, time, event, groups, covar, _, top = _top_hit()
    runs = [S.Backend.last]
    hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=[top], _backend=S.Backend)
    runs.append(S.Backend.last)
    hla, time, event, groups, covar = S.hla_of("n257")
    hb.hlaAssocSurv(hla, time, event, covar, model="genotype", ties="breslow", _backend=S.Backend)
    runs.append(S.Backend.last)
    for r in runs:
        assert all(abs(c - 1e-9) > 1e-15 for crits in r["crit"] for c in crits)


# 5 hlaAssocSurv's host side, on the restatement ------------------------------------------------------------------
def test_result_table_lrt_and_base():
    hla, time, event, groups, covar, res, top = _top_hit()
    r = S.Backend.last
    n, n_allele, q = 1000, 20, 6
    assert res.n_samp == n - 3 and res.n_excluded == 0 and res.n_event == int(r_events(hla, event))
    assert res.name[:n_allele] == S.allele_names(n_allele) and res.name[n_allele:] == ["pos:x", "pos:gap", "pos:y", "pos:z", "pos:beyond"]
    assert (res.n == n - 3).all() and (res.events == res.n_event).all()
    rows = list(range(1, n_allele + 5)) + [-1]
    for t, row in enumerate(rows):
        if row < 0 or r["flags"][row] & 2:
            assert res.flags[t] == 2 and np.isnan(res.est[t, 0]) and np.isnan(res.pval[t, 0]) and np.isnan(res.lrt_p[t]) and np.isnan(res.score_p[t])
            continue
        est, se = r["coef"][row, 0], r["se"][row, 0]
        assert res.est[t, 0] == est and res.se[t, 0] == se and res.iterations[t] == r["iterations"][row]
        assert res.lower[t, 0] == est - 1.959963984540054 * se and res.upper[t, 0] == est + 1.959963984540054 * se
        assert res.pval[t, 0] == math.erfc(abs(est / se) / math.sqrt(2.0))
        stat = 2.0 * (r["loglik"][row] - r["loglik"][0])
        assert res.lrt_stat[t] == stat and res.lrt_p[t] == AR.chisq_p(max(stat, 0.0), 1)
        assert res.score_stat[t] == r["score"][row] and res.score_p[t] == AR.chisq_p(r["score"][row], 1)
        assert res.loglik[t] == r["loglik"][row]
        # Wald, likelihood-ratio and score tests agree roughly for these well-conditioned fits (to a tenth of the exponent)
        for p in (res.lrt_p[t], res.score_p[t]):
            assert abs(math.log10(res.pval[t, 0]) - math.log10(p)) < 0.5 + 0.1 * abs(math.log10(p)) or res.pval[t, 0] > 0.05
        assert 0 < res.carrier_events[t, 0] <= res.carriers[t, 0] < res.n_samp
    assert res.flags[n_allele + 1] == 2 and res.flags[-1] == 2                     # the empty level, the unknown level
    assert res.carriers[n_allele + 1, 0] == 0 and res.carriers[-1, 0] == 0
    assert res.name.index(top) in (0, 1)                                          # a planted allele
    base = res.base
    assert base["name"] == [f"c{j + 1}" for j in range(q)] and base["flags"] == 0 and base["iterations"] >= 2
    assert np.array_equal(base["est"], r["coef"][0, 2:2 + q]) and base["loglik"] == r["loglik"][0]
    assert list(res.to_table()) == ["n", "events", "carriers", "carrier_events", "h.est", "h.se", "h.2.5%", "h.97.5%", "h.pval",
                                    "lrt_stat", "lrt_p", "score_stat", "score_p", "loglik", "iterations", "flags"]
    assert repr(res).startswith("HlaAssocSurvResult('dominant', 'efron', 25 tests, 6 covariates, 997 samples with ")
    # show_hr, and covariates by name
    named = {f"pc{j}": covar[:, j] for j in range(q)}
    res_hr = hb.hlaAssocSurv(hla, time, event, named, groups=groups, show_hr=True, _backend=S.Backend)
    assert list(res_hr.to_table())[4:9] == ["h.est_HR", "h.se", "h.2.5%_HR", "h.97.5%_HR", "h.pval"]
    assert np.array_equal(res_hr.est, np.exp(res.est), equal_nan=True) and np.array_equal(res_hr.upper, np.exp(res.upper), equal_nan=True)
    assert np.array_equal(res_hr.pval, res.pval, equal_nan=True) and np.array_equal(res_hr.se, res.se, equal_nan=True)
    assert res_hr.base["name"] == list(named) and np.array_equal(res_hr.base["est"], base["est"])
    # the order of the samples as given does not matter beyond the order inside a tie block
    back = np.arange(len(time))[::-1]
    hla2 = hb.HlaAlleleClass(locus="A", sample_id=[hla.sample_id[i] for i in back], allele1=[hla.allele1[i] for i in back],
                             allele2=[hla.allele2[i] for i in back])
    res2 = hb.hlaAssocSurv(hla2, time[back], event[back], covar[back], groups=groups, _backend=S.Backend)
    assert np.array_equal(res2.flags, res.flags) and np.allclose(res2.est, res.est, rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.array_equal(res2.carriers, res.carriers) and np.array_equal(res2.carrier_events, res.carrier_events)


def r_events(hla, event):
    known = np.array([a is not None and b is not None for a, b in zip(hla.allele1, hla.allele2)])
    return np.asarray(event)[known].sum()


def test_genotype_table_and_threshold():
    hla, time, event, groups, covar = S.hla_of("n257")
    res = hb.hlaAssocSurv(hla, time, event, covar, model="genotype", ties="breslow", _backend=S.Backend)
    r = S.Backend.last
    cols = list(res.to_table())
    assert cols[2:9] == ["h1.carriers", "h1.carrier_events", "h1.est", "h1.se", "h1.2.5%", "h1.97.5%", "h1.pval"] and cols[9] == "h2.carriers"
    assert np.array_equal(res.est, r["coef"][1:, 0:2], equal_nan=True) and res.est.shape == (12, 2) and res.ties == "breslow"
    both = np.isfinite(res.est).all(axis=1)
    one = np.isfinite(res.est).sum(axis=1) == 1
    assert both.any()
    for t in np.flatnonzero(both | one):
        stat = max(2.0 * (r["loglik"][1 + t] - r["loglik"][0]), 0.0)
        assert res.lrt_p[t] == AR.chisq_p(stat, 2 if both[t] else 1)
        assert res.score_p[t] == AR.chisq_p(r["score"][1 + t], 2 if both[t] else 1)
    # a fit that ran into maxit keeps its likelihood-ratio test (item 7)
    slow = hb.hlaAssocSurv(hla, time, event, covar, maxit=2, _backend=S.Backend)
    assert (slow.flags & 1).any() and np.isfinite(slow.lrt_p[(slow.flags & 1) != 0]).all()
    # a call threshold drops samples, their times and their covariates alike
    prob = np.linspace(0.2, 1.0, len(time))
    withp = hb.HlaAlleleClass(locus="A", sample_id=list(hla.sample_id), allele1=list(hla.allele1), allele2=list(hla.allele2), prob=prob)
    thr = hb.hlaAssocSurv(withp, time, event, covar, prob_threshold=0.5, _backend=S.Backend)
    assert thr.n_excluded == int((prob < 0.5).sum()) and thr.n_samp < res.n_samp


def test_condition():
    hla, time, event, groups, covar, res, top = _top_hit()
    cond = hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=[top], _backend=S.Backend)
    t = res.name.index(top)
    assert cond.flags[t] & 2 and np.isnan(cond.est[t, 0])                          # the conditioned test itself
    assert cond.base["name"][-1] == f"h[{top}]"
    # the base model of the conditioned scan is the top hit's own fit
    assert abs(cond.base["est"][-1] - res.est[t, 0]) <= 1e-6 and abs(cond.base["loglik"] - res.loglik[t]) <= 1e-6
    other = [i for i in range(len(res.name)) if i != t and res.flags[i] == 0 and cond.flags[i] == 0]
    assert len(other) >= 10 and not np.allclose(cond.est[other, 0], res.est[other, 0])
    with pytest.raises(ValueError, match="not a test"):
        hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=["99:99"], _backend=S.Backend)
    with pytest.raises(ValueError, match="no allele of the data"):
        hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=["pos:beyond"], _backend=S.Backend)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocSurv(hla, time, event, np.zeros((len(time), 12)), condition=[top], _backend=S.Backend)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocSurv(hla, time, event, covar, model="genotype", condition=res.name[:4], _backend=S.Backend)


def test_value_errors():
    hla, time, event, groups, covar = S.hla_of("n40")
    n = len(time)
    B = S.Backend
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaAssocSurv(hla, time, event, model="dominent", _backend=B)
    with pytest.raises(ValueError, match="'ties' should be one of"):
        hb.hlaAssocSurv(hla, time, event, ties="exact", _backend=B)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="maxit"):
            hb.hlaAssocSurv(hla, time, event, maxit=bad, _backend=B)
    for bad in (0, -1e-8, math.nan):
        with pytest.raises(ValueError, match="epsilon"):
            hb.hlaAssocSurv(hla, time, event, epsilon=bad, _backend=B)
    kept = [i for i in range(n) if hla.allele1[i] is not None and hla.allele2[i] is not None]
    dropped = [i for i in range(n) if i not in kept]
    for bad in (math.nan, math.inf, -0.5, None, "3"):
        tt = list(time)
        tt[kept[2]] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            hb.hlaAssocSurv(hla, tt, event, _backend=B)
    for bad in (2, -1, 0.5, math.nan, None, "yes"):
        ee = list(event)
        ee[kept[3]] = bad
        with pytest.raises(ValueError, match="0 / 1 or bool"):
            hb.hlaAssocSurv(hla, time, ee, _backend=B)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocSurv(hla, time[:-1], event, _backend=B)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocSurv(hla, time, event[:-1], _backend=B)
    # what a sample that is not kept holds is nobody's business; bool events are events
    tt, ee = list(time), [bool(v) for v in event]
    tt[dropped[0]], ee[dropped[1]] = math.nan, None
    assert hb.hlaAssocSurv(hla, tt, ee, _backend=B).n_samp == n - 3
    c = np.random.default_rng(0).standard_normal((n, 2))
    cc = c.copy()
    cc[kept[7], 1] = math.nan
    with pytest.raises(ValueError, match="'c2'.*non-finite"):
        hb.hlaAssocSurv(hla, time, event, cc, _backend=B)
    with pytest.raises(ValueError, match="values for"):
        hb.hlaAssocSurv(hla, time, event, c[:-1], _backend=B)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocSurv(hla, time, event, np.zeros((n, 13)), _backend=B)
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocSurv(hla, time, event, np.column_stack([c[:, 0], 2 * c[:, 0]]), _backend=B)
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaAssocSurv([1, 2], time, event, _backend=B)
    with pytest.raises(TypeError):
        hb.hlaAssocSurv(hla, time, event, use_prob=True, _backend=B)          # not offered
    # no event at all: every test has bit 1, nothing is raised
    none = hb.hlaAssocSurv(hla, time, np.zeros(n, int), c, _backend=B)
    assert (none.flags == 2).all() and none.n_event == 0 and np.isnan(none.lrt_p).all() and none.base["flags"] == 2


def test_cox_entries_are_declared():
    from hibag_amd import _lib
    for name in ("hibag_hip_assoc_cox", "hibag_hip_assoc_cox_segment"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert "hlaAssocSurv" in hb.__all__ and "HlaAssocSurvResult" in hb.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hibag_hip.h")).read()
    assert f"#define HIBAG_HIP_COX_MAX_COVAR {assocsurv.MAX_COVAR}" in hdr
    assert assoc.MODELS == S.MODELS and assocsurv.TIES == S.TIES
    assert (assocsurv.FLAG_MAXIT, assocsurv.FLAG_RANK, assocsurv.FLAG_CLAMP, assocsurv.FLAG_DECREASE) == \
        (S.MAXIT_BIT, S.RANK_BIT, S.CLAMP_BIT, S.DECREASE_BIT)
    assert S.segment_of(1000) == (4, 128) and S.segment_of(40) == (4, 16)
