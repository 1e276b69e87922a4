"""hlaAssocGlm on the host: the restatement of DESIGN.md section 23 (tests/assocglm_reference.py) against the closed-form
2 x 2 estimate and against an independent scipy.optimize maximum of the likelihood; prior weights, the columns that cannot
be fitted, maxit; hlaAssocGlm's own host side (condition, show_or, the likelihood-ratio test, the base table, every
ValueError) driven by the restatement in place of the device; and the safety condition of the device tests."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_reference as AR  # noqa: E402
import assocglm_reference as G  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assoc, assocglm  # noqa: E402

EST_BOUND, SE_BOUND = 1e-5, 5e-3           # against an exact maximum: the IRLS's stopping error and the se rule of item 5


def _gap(got_est, got_se, want_est, want_se):
    return abs(got_est - want_est) / max(abs(want_est), want_se), abs(got_se / want_se - 1.0)


# 1 closed form ---------------------------------------------------------------------------------------------------
def test_closed_form_2x2():
    """y ~ h, dominant, no covariates: est = the log odds ratio of the 2 x 2 table, se = sqrt(sum of 1 / cell).  Measured:
    est within 3.0e-06 of it in units of max(|est|, se), se within 9.3e-04 relative (both at 40 samples)."""
    worst = [0.0, 0.0]
    seen = 0
    for case in ("n40", "n255", "n1000"):
        n, n_allele, _, seed, _ = G.CASES[case]
        a1, a2, y, _, _, _ = G.cohort(n, n_allele, 0, seed)
        A = AR.Analysis(a1, a2, y, n_allele, None, "dominant")
        r = G.glm_rows(A.F, "dominant", None, None, A.y)
        for t in range(A.n_tests):
            c00, c01, c10, c11 = (float(v) for v in A.tab[t, :4])
            if min(c00, c01, c10, c11) == 0:
                continue
            est, se = math.log(c11 * c00 / (c10 * c01)), math.sqrt(1 / c00 + 1 / c01 + 1 / c10 + 1 / c11)
            assert r["flags"][t] == 0
            ge, gs = _gap(r["coef"][t, 1], r["se"][t, 1], est, se)
            worst = [max(worst[0], ge), max(worst[1], gs)]
            assert ge <= EST_BOUND and gs <= SE_BOUND, (case, t, ge, gs)
            seen += 1
    assert seen >= 20
    print(f"closed form: est {worst[0]:.3g}, se {worst[1]:.3g} over {seen} fits")


# 2 an independent maximum of the likelihood ----------------------------------------------------------------------
def _mle(X, y):
    optimize = pytest.importorskip("scipy.optimize")

    def nll(b):
        eta = X @ b
        return float(np.sum(np.logaddexp(0.0, eta) - y * eta))

    def grad(b):
        return X.T @ (1.0 / (1.0 + np.exp(-(X @ b))) - y)

    def hess(b):
        mu = 1.0 / (1.0 + np.exp(-(X @ b)))
        return X.T @ (X * (mu * (1 - mu))[:, None])

    b = optimize.minimize(nll, np.zeros(X.shape[1]), jac=grad, hess=hess, method="trust-exact", options={"gtol": 1e-12}).x
    for _ in range(3):                                          # Newton steps at the optimum: the gradient down to rounding
        b = b - np.linalg.solve(hess(b), grad(b))
    assert np.linalg.norm(grad(b)) <= 1e-10
    return b, np.sqrt(np.diag(np.linalg.inv(hess(b))))


@pytest.mark.parametrize("model", G.MODELS)
def test_against_an_independent_mle(model):
    """Fits of at most 8 iterations (the near-separated ones are left out and counted).  Measured over the four models:
    est within 2.4e-09 in units of max(|est|, se), se within 4.3e-05 relative."""
    worst = [0.0, 0.0]
    seen = left_out = 0
    for case in ("n255", "n256", "n1000"):
        n, n_allele, q, seed, part = G.CASES[case]
        a1, a2, y, g, covar, _ = G.cohort(n, n_allele, q, seed, part)
        covar, = G.kept_columns(a1, a2, covar)
        A = AR.Analysis(a1, a2, y, n_allele, g, model)
        r = G.reference(case, model)
        slots = G.fit_slots(A.F, A.rsum, model, A.n) + [(-1, -1)]
        for f, rows in enumerate(slots):
            if rows is None or r["flags"][f] & G.RANK_BIT:
                continue
            if r["iterations"][f] > 8:
                left_out += 1
                continue
            used = [0] + [1 + i for i, row in enumerate(rows) if row >= 0] + list(range(G.COV0, G.COV0 + q))
            X = np.stack([np.ones(A.n)] + [A.F[row].astype(float) for row in rows if row >= 0] + list(covar), axis=1)
            b, se = _mle(X, A.y.astype(float))
            for j, slot in enumerate(used):
                ge, gs = _gap(r["coef"][f, slot], r["se"][f, slot], b[j], se[j])
                worst = [max(worst[0], ge), max(worst[1], gs)]
                assert ge <= EST_BOUND and gs <= SE_BOUND, (case, model, f, slot, ge, gs)
            seen += 1
    assert seen >= 10 and left_out <= seen
    print(f"{model}: est {worst[0]:.3g}, se {worst[1]:.3g} over {seen} fits, {left_out} near-separated fits left out")


# 3 prior weights -------------------------------------------------------------------------------------------------
def test_weights():
    """A weight of 0 is the sample removed, a weight of 2 the sample twice: the same likelihood, so with epsilon = 1e-13 the
    same fit but for the stopping error (the start values differ, so the paths do): 1e-6."""
    rng = np.random.default_rng(3)
    n = 120
    X = np.column_stack([np.ones(n), rng.integers(0, 2, n), rng.standard_normal(n)])
    y = (rng.random(n) < 1 / (1 + np.exp(-(0.3 * X[:, 1] - 0.5 * X[:, 2])))).astype(float)
    w = np.ones(n)
    w[5], w[17], w[40] = 0.0, 0.0, 2.0
    got = G.fit(X, y, w, epsilon=1e-13)
    keep = np.r_[np.flatnonzero(w > 0), 40]
    want = G.fit(X[keep], y[keep], np.ones(len(keep)), epsilon=1e-13)
    assert got["flags"] == 0 and want["flags"] == 0
    for k in ("coef", "se"):
        assert np.allclose(got[k], want[k], rtol=1e-6, atol=0), k
    assert abs(got["deviance"] - want["deviance"]) <= 1e-9 * want["deviance"]
    frac = G.fit(X, y, rng.uniform(0.2, 1.0, n))
    assert frac["flags"] == 0 and np.isfinite(frac["se"]).all()


# 4 columns that cannot be fitted ---------------------------------------------------------------------------------
def test_unfittable_columns():
    n = 30
    rng = np.random.default_rng(4)
    y = rng.integers(0, 2, n)
    zero, one, two = np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2, np.int64)
    some = (np.arange(n) % 3 == 0).astype(np.int64)
    few = (np.arange(n) % 7 == 1).astype(np.int64)
    for model, F, want in (("dominant", np.stack([zero, one, some]), [2, 2, 0]),
                           ("recessive", np.stack([zero, one, some]), [2, 2, 0]),
                           ("additive", np.stack([zero, two, one, some + few]), [2, 2, 2, 0])):     # all het: the pivot rule
        r = G.glm_rows(F, model, None, None, y)
        assert (r["flags"][:-1] & 3).tolist() == want, model
        for t, fl in enumerate(want):
            assert np.isnan(r["coef"][t]).all() == (fl == 2) and np.isnan(r["deviance"][t]) == (fl == 2)
    # genotype: rows (het, hom) per test -- both empty; nobody without; no hom; no het; both
    F = np.stack([zero, zero, some, 1 - some, some, zero, zero, few, some, few])
    r = G.glm_rows(F, "genotype", None, None, y)
    assert (r["flags"][:-1] & 2).tolist() == [2, 2, 0, 0, 0]
    fitted = np.isfinite(r["coef"][:-1, 1:3])
    assert fitted.tolist() == [[False, False], [False, False], [True, False], [False, True], [True, True]]
    assert np.array_equal(np.isfinite(r["se"][:-1, 1:3]), fitted)
    # the one fitted dummy is the single-column fit of that row
    alone = G.glm_rows(some[None, :], "dominant", None, None, y)
    assert r["coef"][2, 1] == alone["coef"][0, 1] and r["se"][2, 1] == alone["se"][0, 1]
    assert np.isfinite(r["coef"][-1, 0]) and np.isnan(r["coef"][-1, 1:]).all()          # the base model: the intercept alone
    # a covariate equal to a test's column: the pivot rule
    r = G.glm_rows(np.stack([some, few]), "dominant", some[None, :].astype(float), None, y)
    assert (r["flags"] & 2).tolist() == [2, 0, 0]


def test_maxit_2_sets_bit_0_everywhere():
    for model in G.MODELS:
        r = G.reference("n257", model, maxit=2)
        fitted = (r["flags"] & G.RANK_BIT) == 0
        assert fitted.any() and ((r["flags"][fitted] & G.MAXIT_BIT) != 0).all() and (r["iterations"][fitted] == 2).all()
        assert np.isfinite(r["coef"][fitted, 0]).all() and np.isfinite(r["deviance"][fitted]).all()


# 5 the safety condition of the device tests ----------------------------------------------------------------------
@pytest.mark.parametrize("run", G.DEVICE_RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_no_criterion_near_epsilon(run):
    """No convergence criterion of any compared fit lies within 1e-6 (relative) of epsilon, so that a device whose sums
    differ in the last bits takes the same number of iterations; and the tolerance of the device tests exists."""
    r = G.reference(*run)
    for f, crits in enumerate(r["crit"]):
        for c in crits:
            assert abs(c - 1e-8) > 1e-6 * 1e-8, (run, f, c)
    assert 1e-12 <= G.tolerance(*run) <= 1e-6, G.tolerance(*run)


def _top_hit(case="n1000"):
    hla, y, groups, covar = G.hla_of(case)
    res = hb.hlaAssocGlm(hla, y, covar, groups=groups, _backend=G.Backend)
    return hla, y, groups, covar, res, res.name[int(np.nanargmin(res.pval[:, 0]))]


def test_no_criterion_near_epsilon_conditioned():
    """The same for the end-to-end run of the device tests: n1000, dominant, conditioned on its top hit."""
    hla, y, groups, covar, _, top = _top_hit()

    class Recording(G.Backend):
        def glm(self, *args):
            r = G.glm_rows(self.A.F, self.model, args[0], args[1], self.A.y, args[2], args[3])
            Recording.crit = r["crit"]
            return r["coef"], r["se"], r["deviance"], r["iterations"], r["flags"]

    hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=[top], _backend=Recording)
    assert all(abs(c - 1e-8) > 1e-14 for crits in Recording.crit for c in crits)


# 6 hlaAssocGlm's host side, on the restatement -------------------------------------------------------------------
def test_result_table_lrt_and_base():
    hla, y, groups, covar, res, top = _top_hit()
    n, n_allele, q, _, _ = G.CASES["n1000"]
    r = G.reference("n1000", "dominant")
    assert res.n_samp == n - 3 and res.n_excluded == 0 and res.n_case == int(res.n_case)
    assert res.name[:n_allele] == G.allele_names(n_allele) and res.name[n_allele:] == ["pos:x", "pos:gap", "pos:y", "pos:z", "pos:beyond"]
    rows = list(range(n_allele + 4)) + [-1]
    for t, row in enumerate(rows):
        if row < 0 or r["flags"][row] & 2:
            assert res.flags[t] == 2 and np.isnan(res.est[t, 0]) and np.isnan(res.pval[t, 0]) and np.isnan(res.lrt_p[t])
            continue
        est, se = r["coef"][row, 1], r["se"][row, 1]
        assert res.est[t, 0] == est and res.se[t, 0] == se and res.iterations[t] == r["iterations"][row]
        assert res.lower[t, 0] == est - 1.959963984540054 * se and res.upper[t, 0] == est + 1.959963984540054 * se
        assert res.pval[t, 0] == math.erfc(abs(est / se) / math.sqrt(2.0))
        stat = r["deviance"][-1] - r["deviance"][row]
        assert res.lrt_stat[t] == stat and res.lrt_p[t] == AR.chisq_p(max(stat, 0.0), 1)
        # Wald and likelihood-ratio tests agree roughly for these well-conditioned fits
        assert abs(math.log10(res.pval[t, 0]) - math.log10(res.lrt_p[t])) < 0.5 or res.pval[t, 0] > 0.05
    assert res.flags[n_allele + 1] == 2 and res.flags[-1] == 2                     # the empty level, the unknown level
    assert res.name.index(top) in (0, 1)                                          # a planted allele
    base = res.base
    assert base["name"] == ["(Intercept)"] + [f"c{j + 1}" for j in range(q)] and base["flags"] == 0
    assert np.array_equal(base["est"], r["coef"][-1, [0] + list(range(3, 3 + q))]) and base["deviance"] == r["deviance"][-1]
    assert list(res.to_table()) == ["h.est", "h.2.5%", "h.97.5%", "h.pval"]
    # show_or, and covariates by name
    named = {f"pc{j}": covar[:, j] for j in range(q)}
    res_or = hb.hlaAssocGlm(hla, y, named, groups=groups, show_or=True, _backend=G.Backend)
    assert list(res_or.to_table()) == ["h.est_OR", "h.2.5%_OR", "h.97.5%_OR", "h.pval"]
    assert np.array_equal(res_or.est, np.exp(res.est), equal_nan=True) and np.array_equal(res_or.upper, np.exp(res.upper), equal_nan=True)
    assert np.array_equal(res_or.pval, res.pval, equal_nan=True) and np.array_equal(res_or.se, res.se, equal_nan=True)
    assert res_or.base["name"][1:] == list(named) and np.array_equal(res_or.base["est"], base["est"])


def test_genotype_table_and_use_prob():
    hla, y, groups, covar = G.hla_of("n257")
    res = hb.hlaAssocGlm(hla, y, covar, model="genotype", use_prob=True, _backend=G.Backend)
    r = G.reference("n257", "genotype", weighted=True)
    assert list(res.to_table()) == [f"{h}.{c}" for h in ("h1", "h2") for c in ("est", "2.5%", "97.5%", "pval")]
    assert np.array_equal(res.est, r["coef"][:-1, 1:3], equal_nan=True) and res.est.shape == (12, 2)
    both = np.isfinite(res.est).all(axis=1) & (res.flags == 0)
    one = (np.isfinite(res.est).sum(axis=1) == 1) & (res.flags == 0)
    assert both.any()
    for t in np.flatnonzero(both | one):
        stat = max(r["deviance"][-1] - r["deviance"][t], 0.0)
        assert res.lrt_p[t] == AR.chisq_p(stat, 2 if both[t] else 1)
    # a call threshold drops samples and their covariates alike
    thr = hb.hlaAssocGlm(hla, y, covar, prob_threshold=0.5, _backend=G.Backend)
    assert thr.n_excluded == int((np.asarray(hla.prob) < 0.5).sum()) and thr.n_samp < res.n_samp


def test_condition():
    hla, y, groups, covar, res, top = _top_hit()
    cond = hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=[top], _backend=G.Backend)
    t = res.name.index(top)
    assert cond.flags[t] & 2 and np.isnan(cond.est[t, 0])                          # the conditioned test itself
    assert cond.base["name"][-1] == f"h[{top}]"
    # the base model of the conditioned scan is the top hit's own fit
    assert abs(cond.base["est"][-1] - res.est[t, 0]) <= 1e-6 and abs(cond.base["deviance"] - res.deviance[t]) <= 1e-6
    other = [i for i in range(len(res.name)) if i != t and res.flags[i] == 0 and cond.flags[i] == 0]
    assert len(other) >= 10 and not np.allclose(cond.est[other, 0], res.est[other, 0])
    # by hand: the column of the top hit among the covariates
    n, n_allele, q, seed, part = G.CASES["n1000"]
    a1, a2, yy, g, cv, _ = G.cohort(n, n_allele, q, seed, part)
    cv, = G.kept_columns(a1, a2, cv)
    A = AR.Analysis(a1, a2, yy, n_allele, g, "dominant")
    want = G.glm_rows(A.F, "dominant", np.concatenate([cv, A.F[t][None, :].astype(float)]), None, A.y)
    assert np.array_equal(cond.est[:n_allele, 0], want["coef"][:n_allele, 1], equal_nan=True)
    with pytest.raises(ValueError, match="not a test"):
        hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=["99:99"], _backend=G.Backend)
    with pytest.raises(ValueError, match="no allele of the data"):
        hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=["pos:beyond"], _backend=G.Backend)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocGlm(hla, y, np.zeros((len(y), 12)), condition=[top], _backend=G.Backend)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocGlm(hla, y, covar, model="genotype", condition=res.name[:4], _backend=G.Backend)


def test_value_errors():
    hla, y, groups, covar = G.hla_of("n40")
    n = len(y)
    B = G.Backend
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaAssocGlm(hla, y, model="dominent", _backend=B)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="maxit"):
            hb.hlaAssocGlm(hla, y, maxit=bad, _backend=B)
    for bad in (0, -1e-8, math.nan):
        with pytest.raises(ValueError, match="epsilon"):
            hb.hlaAssocGlm(hla, y, epsilon=bad, _backend=B)
    c = np.random.default_rng(0).standard_normal((n, 2))
    for bad in (math.nan, math.inf):
        cc = c.copy()
        cc[7, 1] = bad
        with pytest.raises(ValueError, match="'c2'.*non-finite"):
            hb.hlaAssocGlm(hla, y, cc, _backend=B)
    with pytest.raises(ValueError, match="values for"):
        hb.hlaAssocGlm(hla, y, c[:-1], _backend=B)
    with pytest.raises(ValueError, match="values for"):
        hb.hlaAssocGlm(hla, y, {"age": c[:-1, 0]}, _backend=B)
    with pytest.raises(ValueError, match="array"):
        hb.hlaAssocGlm(hla, y, np.zeros((n, 1, 1)), _backend=B)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocGlm(hla, y, np.zeros((n, 13)), _backend=B)
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocGlm(hla, y, np.column_stack([c[:, 0], 2 * c[:, 0]]), _backend=B)
    no_prob = hb.HlaAlleleClass(locus="A", sample_id=list(hla.sample_id), allele1=list(hla.allele1), allele2=list(hla.allele2))
    with pytest.raises(ValueError, match="posterior probability"):
        hb.hlaAssocGlm(no_prob, y, use_prob=True, _backend=B)
    for bad in (-0.1, math.nan):
        prob = np.array(hla.prob, float)
        prob[3] = bad
        worse = hb.HlaAlleleClass(locus="A", sample_id=list(hla.sample_id), allele1=list(hla.allele1), allele2=list(hla.allele2), prob=prob)
        with pytest.raises(ValueError, match="finite and >= 0"):
            hb.hlaAssocGlm(worse, y, use_prob=True, _backend=B)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocGlm(hla, y[:-1], _backend=B)
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaAssocGlm([1, 2], y, _backend=B)
    # a non-finite covariate of a sample that is not kept is nobody's business
    dropped = [i for i, a in enumerate(hla.allele1) if a is None or hla.allele2[i] is None]
    cc = c.copy()
    cc[dropped[0], 0] = math.nan
    assert hb.hlaAssocGlm(hla, y, cc, _backend=B).n_samp == n - 3


def test_glm_entries_are_declared():
    from hibag_amd import _lib
    for name in ("hibag_hip_assoc_n_kept", "hibag_hip_assoc_feature_rows", "hibag_hip_assoc_glm"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert "hlaAssocGlm" in hb.__all__ and "HlaAssocGlmResult" in hb.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hibag_hip.h")).read()
    assert f"#define HIBAG_HIP_GLM_MAX_COVAR {assocglm.MAX_COVAR}" in hdr
    assert assoc.MODELS == G.MODELS
