"""hlaAssocOmnibus on the host: the restatement of DESIGN.md section 26 (tests/assocomni_reference.py) against section 23's
one-column fit, against an independent scipy.optimize maximum of the likelihood, under a change of the reference level and
with exactly collinear columns; the chi-square tail against scipy.stats; hlaAssocOmnibus's and hlaAssocStepwise's own host
side driven by the restatement in place of the device; and the safety conditions of the device tests."""

import math
import os
import sys

import numpy as np
import pytest
import scipy.optimize
import scipy.stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assocglm_reference as G  # noqa: E402
import assocomni_reference as O  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, assocomni  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def omnibus(case, q=6, **kw):
    hla, y, groups, covar = O.hla_of(case)
    return hb.hlaAssocOmnibus(hla, y, groups, covar[:, :q] if q else None, _backend=O.Backend, **kw)


def design(case, model, rows, q):
    """X = [1 | rows | the first q covariates], y, the weights 1."""
    A, covar, _, _ = O.analysis(case, model)
    X = np.stack([np.ones(A.n)] + [A.F[r].astype(float) for r in rows] + list(covar[:q]), axis=1)
    return X, A.y.astype(float), np.ones(A.n)


# 1 the fit -------------------------------------------------------------------------------------------------------
def test_a_one_row_set_is_the_fit_of_section_23():
    """The same columns through tests/assocglm_reference.py: the factorisation order differs (the row before the covariates
    there, after them here), nothing else: 1e-12."""
    seen = 0
    for case, model, q in (("n257", "additive", 12), ("n1000", "dominant", 6), ("n40", "additive", 0)):
        A = O.analysis(case, model)[0]
        for t in range(O.CASES[case][1]):
            if A.rsum[t] < 5:
                continue
            X, y, w = design(case, model, [t], q)
            got, want = O.fit(X, 1, y, w), G.fit(X, y, w)
            assert got["flags"] == want["flags"] == 0 and got["iterations"] == want["iterations"] and got["df_h"] == 1
            scale = np.fmax(np.abs(want["coef"]), want["se"])
            assert (np.abs(got["coef"] - want["coef"]) <= 1e-12 * scale).all() and np.allclose(got["se"], want["se"], rtol=1e-12, atol=0)
            assert abs(got["deviance"] / want["deviance"] - 1) <= 1e-12
            seen += 1
    assert seen >= 20


def _mle(X, y):
    optimize = scipy.optimize

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
    assert np.linalg.norm(grad(b)) <= 1e-9
    return b, np.sqrt(np.diag(np.linalg.inv(hess(b)))), 2.0 * nll(b)


def test_against_an_independent_mle():
    """Every partition's set of the 1000- and 256-sample cohorts (fits without a flag, of at most 8 iterations): deviance and
    likelihood-ratio statistic within 1e-8 relative, se within 5e-3 (section 23 item 5: the weights of the last solve).
    Measured: deviance 2.2e-16, LRT 6.4e-14, se 1.8e-5, est 2.7e-9 (units of max(|est|, se)) over 11 fits."""
    worst = [0.0, 0.0, 0.0, 0.0]
    seen = 0
    for case, q in (("n1000", 6), ("n256", 5)):
        A, covar, _, part_rows = O.analysis(case, "additive")
        sets = [[rows[lv] for lv in s] for rows, s in zip(part_rows, O.design_sets(part_rows, A.rsum)[0])]
        r = O.glm_sets(A.F, sets, covar[:q], None, A.y)
        _, _, base_dev = _mle(design(case, "additive", [], q)[0], A.y.astype(float))
        assert abs(r["deviance"][-1] / base_dev - 1) <= 1e-8
        for f, s in enumerate(sets):
            if r["flags"][f] != 0 or r["iterations"][f] > 8:
                continue
            X, y, _ = design(case, "additive", s, q)
            b, se, dev = _mle(X, y)
            slots = [0] + list(range(1, 1 + len(s))) + list(range(1 + r["H"], 1 + r["H"] + q))
            lrt, want_lrt = r["deviance"][-1] - r["deviance"][f], base_dev - dev
            gaps = [abs(r["deviance"][f] / dev - 1), abs(lrt / want_lrt - 1), float(np.max(np.abs(r["se"][f, slots] / se - 1))),
                    float(np.max(np.abs(r["coef"][f, slots] - b) / np.fmax(np.abs(b), se)))]
            worst = [max(a, g) for a, g in zip(worst, gaps)]
            assert gaps[0] <= 1e-8 and gaps[1] <= 1e-8 and gaps[2] <= 5e-3 and gaps[3] <= 1e-5, (case, f, gaps)
            seen += 1
    assert seen >= 8
    print(f"independent maximum: deviance {worst[0]:.3g}, LRT {worst[1]:.3g}, se {worst[2]:.3g}, est {worst[3]:.3g} over {seen} fits")


def test_the_reference_level_does_not_matter():
    """Leaving out another level is the same model: deviance and LRT within 1e-9 relative."""
    A, covar, _, part_rows = O.analysis("n1000", "additive")
    base = O.glm_sets(A.F, [], covar[:6], None, A.y)["deviance"][-1]
    for p in (1, 2, 3):                                         # p3, p5, p8
        rows = [r for r in part_rows[p] if A.rsum[r] > 0]
        devs = []
        for ref in rows:
            X, y, w = design("n1000", "additive", [r for r in rows if r != ref], 6)
            res = O.fit(X, len(rows) - 1, y, w)
            assert res["flags"] == 0 and res["df_h"] == len(rows) - 1
            devs.append(float(res["deviance"]))
        devs = np.array(devs)
        assert np.max(np.abs(devs / devs[0] - 1)) <= 1e-9 and np.max(np.abs((base - devs) / (base - devs[0]) - 1)) <= 1e-9


# 2 aliased columns -----------------------------------------------------------------------------------------------
def assert_equals_fit_without(res, X, n_h, y, w, dropped):
    keep = [j for j in range(X.shape[1]) if j not in dropped]
    want = O.fit(X[:, keep], n_h - sum(1 for j in dropped if 1 <= j <= n_h), y, w)
    assert want["flags"] == 0 and res["flags"] == O.ALIASED_BIT and res["iterations"] == want["iterations"]
    assert np.isnan(res["coef"][dropped]).all() and np.isnan(res["se"][dropped]).all()
    assert np.allclose(res["coef"][keep], want["coef"], rtol=1e-10, atol=1e-13) and np.allclose(res["se"][keep], want["se"], rtol=1e-10, atol=0)
    assert abs(res["deviance"] / want["deviance"] - 1) <= 1e-12 and res["df_h"] == want["df_h"]


def test_a_level_equal_to_a_covariate_is_dropped():
    """The covariates come first in the factorisation, so of two equal columns the level's is the aliased one."""
    A, covar, _, part_rows = O.analysis("n1000", "additive")
    rows = part_rows[2][1:4]                                    # three levels of p5
    X, y, w = design("n1000", "additive", rows, 3)
    X = np.column_stack([X, A.F[rows[1]].astype(float)])        # a fourth covariate: the second level
    res = O.fit(X, 3, y, w)
    assert res["df_h"] == 2 and np.isfinite(res["coef"][[0, 1, 3, 4, 5, 6, 7]]).all()
    assert_equals_fit_without(res, X, 3, y, w, [2])
    assert min(abs(v) for v in res["ratios"] if v < 1e-9) < 1e-13


def test_levels_that_add_up_to_the_intercept():
    """All levels of a partition, additive: they add up to 2, and the last one in the factorisation goes."""
    rows = O.analysis("n1000", "additive")[3][2]                # p5
    X, y, w = design("n1000", "additive", rows, 6)
    res = O.fit(X, 5, y, w)
    assert res["df_h"] == 4
    assert_equals_fit_without(res, X, 5, y, w, [5])


def test_a_partition_that_repeats_the_conditioned_one():
    """p3b has the levels of p3 under other numbers: with p3's columns among the covariates every column of p3b -- and of p3
    itself -- is aliased: df 0, the base model's deviance, no p-value."""
    r = omnibus("n1000", condition=["p3"])
    assert r.base["name"][-2:] == ["h[p3:p3.1]", "h[p3:p3.2]"] and r.base["flags"] == 0 and np.isfinite(r.base["est"]).all()
    for name in ("p3", "p3b"):
        i = r.name.index(name)
        assert r.flags[i] == O.ALIASED_BIT and r.df[i] == 0 and np.isnan(r.lrt_p[i]) and np.isnan(r.est[i]).all() and np.isnan(r.se[i]).all()
        assert abs(r.deviance[i] / r.base["deviance"] - 1) <= 1e-12 and abs(r.lrt_stat[i]) <= 1e-9
    i = r.name.index("gap")                                     # gap = {level 0 of p3} + two others: one column is p3's
    plain = omnibus("n1000")
    assert plain.df[i] == 2 and r.df[i] == 1 and r.flags[i] == O.ALIASED_BIT and np.isfinite(r.lrt_p[i])
    # the columns that remain are the fit without the aliased one
    A, covar, _, part_rows = O.analysis("n1000", "additive")
    cond = [part_rows[1][1], part_rows[1][2]]
    sets, ref, _ = O.design_sets(part_rows, A.rsum)
    assert ref[1] == 0 and ref[4] == 0 and sets[4] == [2, 3]
    rows = [part_rows[4][lv] for lv in sets[4]]
    X = np.stack([np.ones(A.n)] + [A.F[k].astype(float) for k in rows] + list(covar[:6]) + [A.F[k].astype(float) for k in cond], axis=1)
    res = O.fit(X, 2, A.y.astype(float), np.ones(A.n))
    dropped = [j for j in (1, 2) if np.isnan(res["coef"][j])]
    assert len(dropped) == 1
    assert_equals_fit_without(res, X, 2, A.y.astype(float), np.ones(A.n), dropped)


def test_an_aliased_conditioned_column_is_dropped_from_the_base_model():
    """Conditioning on p3 and on one of its levels again: the repeated column is aliased in the base model, which goes on
    without it and says so; two equal covariates of the user's are a ValueError."""
    r = omnibus("n1000", condition=["p3", "p3:p3.1"])
    assert r.base["name"][-3:] == ["h[p3:p3.1]", "h[p3:p3.2]", "h[p3:p3.1]"] and r.base["flags"] == O.ALIASED_BIT
    assert np.isnan(r.base["est"][-1]) and np.isfinite(r.base["est"][:-1]).all()
    plain = omnibus("n1000", condition=["p3"])
    assert np.allclose(r.base["est"][:-1], plain.base["est"], rtol=1e-10, atol=1e-13) and np.allclose(r.lrt_stat, plain.lrt_stat, rtol=0, atol=1e-8, equal_nan=True)
    hla, y, groups, covar = O.hla_of("n1000")
    twice = np.column_stack([covar[:, :3], covar[:, 1]])
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocOmnibus(hla, y, groups, twice, _backend=O.Backend)


# 3 the chi-square tail -------------------------------------------------------------------------------------------
def test_chisq_tail():
    stats = scipy.stats
    xs = np.concatenate([np.geomspace(1e-3, 200, 400), [1e-3, 1.0, 30.0, 200.0]])
    worst = 0.0
    for df in range(1, 31):
        want = stats.chi2.sf(xs, df)
        got = np.array([assocomni.chisq_sf(float(x), df) for x in xs])
        ref = np.array([O.chisq_sf(float(x), df) for x in xs])
        worst = max(worst, float(np.max(np.abs(got / want - 1))), float(np.max(np.abs(ref / want - 1))))
    print(f"chi-square tail: {worst:.3g} relative")
    assert worst <= 1e-12
    assert assocomni.chisq_sf(-1e-9, 3) == 1.0 and math.isnan(assocomni.chisq_sf(math.nan, 3)) and math.isnan(assocomni.chisq_sf(1.0, 0))
    assert assocomni.chisq_sf(4.0, 1) == math.erfc(math.sqrt(2.0)) and assocomni.chisq_sf(4.0, 2) == math.exp(-2.0)


# 4 hlaAssocOmnibus and hlaAssocStepwise on the restatement -------------------------------------------------------------
def test_result_names_reference_and_columns():
    r = omnibus("n1000")
    A, covar, _, part_rows = O.analysis("n1000", "additive")
    assert r.name == ["p2", "p3", "p5", "p8", "gap", "p3b", "all"] and r.model == "additive" and r.locus == "DRB1"
    assert (r.n_samp, r.n_case, r.n_excluded) == (A.n, A.n_case, 0) and "7 partitions" in repr(r)
    sets, ref, carried = O.design_sets(part_rows, A.rsum)
    assert r.n_levels.tolist() == carried == [2, 3, 5, 8, 3, 3, 24]
    assert r.reference == ["p2.0", "p3.0", "p5.0", "p8.0", "gap.0", "p3b.1", "all.0"]
    want = O.glm_sets(A.F, [[rows[lv] for lv in s] for rows, s in zip(part_rows, sets)], covar[:6], None, A.y)
    assert r.df.tolist() == want["df_h"][:-1].tolist() == [1, 2, 4, 7, 2, 2, 23] and (r.flags == 0).all()
    for p, s in enumerate(sets):
        assert r.level_names[p][:2] == [f"{r.name[p]}.0", f"{r.name[p]}.1"]
        assert np.array_equal(r.est[p][s], want["coef"][p, 1:1 + len(s)]) and np.array_equal(r.se[p][s], want["se"][p, 1:1 + len(s)])
        others = [lv for lv in range(len(r.level_names[p])) if lv not in s]
        assert ref[p] in others and all(np.isnan(getattr(r, k)[p][others]).all() for k in ("est", "se", "lower", "upper", "pval"))
        z = r.est[p][s] / r.se[p][s]
        assert np.allclose(r.pval[p][s], [math.erfc(abs(v) / math.sqrt(2)) for v in z], rtol=1e-14)
        assert np.allclose(r.lower[p][s], r.est[p][s] - 1.959963984540054 * r.se[p][s]) and np.allclose(r.upper[p][s], r.est[p][s] + 1.959963984540054 * r.se[p][s])
        assert r.lrt_stat[p] == want["deviance"][-1] - want["deviance"][p]
        assert abs(r.lrt_p[p] / O.chisq_sf(r.lrt_stat[p], len(s)) - 1) <= 1e-13          # (two ways of adding the same series)
    assert r.level_names[0] == ["p2.0", "p2.1", "p2.beyond"] and np.isnan(r.est[0][2])         # a level the device does not know
    assert r.level_names[4][1] == "gap.1" and np.isnan(r.est[4][1])                            # a level nobody carries
    assert r.base["name"] == ["(Intercept)"] + [f"c{j + 1}" for j in range(6)] and r.base["flags"] == 0
    assert np.array_equal(r.base["est"], want["coef"][-1, [0] + list(range(24, 30))]) and r.base["deviance"] == want["deviance"][-1]
    assert set(r.to_table()) == {"n.levels", "df", "deviance", "lrt.st", "lrt.p"}
    assert r.lrt_p[1] < 1e-30 and int(np.nanargmin(r.lrt_p)) in (1, 5)                         # the planted position


def test_reference_tie_break_and_untested_partitions():
    rsum = np.array([5, 9, 9, 0, 9, 3, 0, 4])
    got = assocomni._design_sets([[0, 1, 2, 3], [4, -1, 5], [6, 7], [3, 6]], rsum)
    assert got == O.design_sets([[0, 1, 2, 3], [4, -1, 5], [6, 7], [3, 6]], rsum)
    assert got == ([[0, 2], [2], [], []], [1, 0, -1, -1], [3, 2, 1, 0])          # the tie of rows 1 and 2 goes to the lower level
    for case in O.CASES:
        A, _, _, part_rows = O.analysis(case, "recessive")
        assert assocomni._design_sets(part_rows, A.rsum) == O.design_sets(part_rows, A.rsum)
    # a partition with one level, beside the others: not tested, bit 1
    hla, y, groups, covar = O.hla_of("n257")
    one = hb.HlaAlleleGroups(groups.alleles, ["one"], [["one.0"]], np.zeros((1, 12), np.int32))
    r = hb.hlaAssocOmnibus(hla, y, groups + one, covar[:, :2], _backend=O.Backend)
    assert r.name[-1] == "one" and r.flags[-1] == O.RANK_BIT and r.reference[-1] is None and r.n_levels[-1] == 1 and r.df[-1] == 0
    assert np.isnan(r.lrt_p[-1]) and np.isnan(r.deviance[-1]) and np.isnan(r.est[-1]).all() and (r.flags[:-1] == 0).all()
    with pytest.raises(ValueError, match="fewer than two levels"):
        hb.hlaAssocOmnibus(hla, y, groups + one, covar[:, :2], condition=["one"], _backend=O.Backend)


def test_a_partition_too_wide_for_the_design():
    r = omnibus("n1000", q=12)
    i = r.name.index("all")
    assert r.flags[i] == O.TOO_WIDE_BIT | O.RANK_BIT and r.df[i] == 0 and np.isnan(r.lrt_p[i]) and np.isnan(r.est[i]).all()
    assert r.reference[i] == "all.0" and r.n_levels[i] == 24 and (r.flags[:i] == 0).all()
    assert r.base["name"][-1] == "c12" and np.isfinite(r.base["est"]).all() and len(r.base["est"]) == 13


def test_models_weights_and_maxit():
    for model in ("dominant", "recessive"):
        r = omnibus("n257", model=model, use_prob=True)
        assert r.model == model and np.isfinite(r.lrt_p[:3]).all()
    r2 = omnibus("n257", maxit=2)
    assert (r2.flags & O.MAXIT_BIT).all() and np.isnan(r2.lrt_p).all() and np.isfinite(r2.est[1][1:]).all()
    hla, y, groups, covar = O.hla_of("n257")
    keep = np.asarray(hla.prob) >= 0.5
    r = hb.hlaAssocOmnibus(hla, y, groups, {"age": covar[:, 0], "sex": covar[:, 1]}, prob_threshold=0.5, _backend=O.Backend)
    assert r.n_excluded == int((~keep).sum()) and r.base["name"] == ["(Intercept)", "age", "sex"]


def test_value_errors():
    hla, y, groups, covar = O.hla_of("n257")
    run = lambda *a, **kw: hb.hlaAssocOmnibus(hla, y, *a, _backend=O.Backend, **kw)          # noqa: E731
    with pytest.raises(ValueError, match="genotype"):
        run(groups, model="genotype")
    with pytest.raises(ValueError, match="should be one of"):
        run(groups, model="allelic")
    with pytest.raises(TypeError, match="HlaAlleleGroups"):
        run(None)
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="maxit"):
            run(groups, maxit=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            run(groups, epsilon=bad)
    c = covar[:, :2].copy()
    c[7, 1] = np.nan
    with pytest.raises(ValueError, match="'c2' has a missing"):
        run(groups, c)
    with pytest.raises(ValueError, match="has 5 values"):
        run(groups, np.zeros((5, 1)))
    with pytest.raises(ValueError, match="list of partition or test names"):
        run(groups, condition=[3])
    with pytest.raises(ValueError, match="neither a partition nor a test"):
        run(groups, condition=["p9"])
    with pytest.raises(ValueError, match="no allele of the data"):
        run(groups, condition=["p2:p2.beyond"])
    with pytest.raises(ValueError, match=r"31 covariate columns \(7 conditioned"):
        run(groups, covar[:, :24], condition=["p8"])
    assert len(run(groups, covar[:, :22], condition=["p8"]).base["name"]) == 30          # 29 columns are fine
    no_prob = hb.HlaAlleleClass(locus="A", sample_id=hla.sample_id, allele1=hla.allele1, allele2=hla.allele2)
    with pytest.raises(ValueError, match="No posterior probability"):
        hb.hlaAssocOmnibus(no_prob, y, groups, use_prob=True, _backend=O.Backend)
    neg = hb.HlaAlleleClass(locus="A", sample_id=hla.sample_id, allele1=hla.allele1, allele2=hla.allele2, prob=-np.asarray(hla.prob))
    with pytest.raises(ValueError, match="finite and >= 0"):
        hb.hlaAssocOmnibus(neg, y, groups, use_prob=True, _backend=O.Backend)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocOmnibus(hla, y[:-1], groups, _backend=O.Backend)
    for kw in ({"max_steps": -1}, {"max_steps": 1.5}, {"p_stop": 2.0}, {"p_stop": float("nan")}):
        with pytest.raises(ValueError, match="max_steps|p_stop"):
            hb.hlaAssocStepwise(hla, y, groups, _backend=O.Backend, **kw)


def test_stepwise_takes_the_planted_position_and_stops():
    hla, y, groups, covar = O.hla_of("n1000", without=("p3b",))
    r = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], _backend=O.Backend)
    assert r.chosen == ["p3"] and len(r.steps) == 2 and r.lrt_p[0] == r.steps[0].lrt_p[1] < 5e-8 and "chosen ['p3']" in repr(r)
    second = r.steps[1]
    assert second.base["name"][-2:] == ["h[p3:p3.1]", "h[p3:p3.2]"] and second.df[1] == 0 and not np.nanmin(second.lrt_p) <= 5e-8
    # a loose threshold goes on; max_steps and the column budget end it
    loose = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], p_stop=0.9, max_steps=2, _backend=O.Backend)
    assert loose.chosen[0] == "p3" and len(loose.chosen) == 2 and len(loose.steps) == 3 and loose.chosen[1] != "p3"
    assert hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], max_steps=0, _backend=O.Backend).chosen == []
    tight = hb.hlaAssocStepwise(hla, y, groups, covar[:, :28], _backend=O.Backend)           # p3 would be columns 29 and 30
    assert tight.chosen == [] and len(tight.steps) == 1 and tight.steps[0].lrt_p[1] < 5e-8
    start = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], condition="p3", _backend=O.Backend)
    assert start.chosen == [] and start.steps[0].base["name"][-1] == "h[p3:p3.2]"


# 5 what the device tests rest on ---------------------------------------------------------------------------------
def test_the_device_runs_cover_the_shapes():
    """Read off the restatement: designs of 15, 16, 17 and 31 columns, both ways of filling 31, no covariate, a set too wide,
    an empty one, a row nobody carries, an exactly aliased row, sets of different sizes in a call."""
    columns = set()
    for run in O.DEVICE_RUNS:
        r, sets = O.reference(*run), O.run_sets(*run[:3])
        fitted = (r["flags"][:-1] & O.RANK_BIT) == 0
        columns |= {(1 + len(s) + run[2], run[2]) for s, ok in zip(sets, fitted) if ok}
        assert len({len(s) for s, ok in zip(sets, fitted) if ok}) >= 2 or run[2] == 29
    assert {c for c, _ in columns} >= {15, 16, 17, 31} and (31, 12) in columns and (31, 29) in columns and any(q == 0 for _, q in columns)
    r = O.reference("n1000", "additive", 12)
    assert (r["flags"] == (O.TOO_WIDE_BIT | O.RANK_BIT)).sum() >= 2 and (r["flags"] == O.RANK_BIT).sum() >= 2
    r, sets = O.reference("n1000", "additive", 6), O.run_sets("n1000", "additive", 6)
    everyone = sets.index(list(range(24)))
    assert r["flags"][everyone] == O.ALIASED_BIT and r["df_h"][everyone] == 23 and np.isnan(r["coef"][everyone, 24])
    assert np.isfinite(r["coef"][everyone, 1:24]).all()
    gap = [i for i, s in enumerate(sets) if len(s) == 3 and r["flags"][i] == O.ALIASED_BIT]
    assert gap and np.isnan(r["coef"][gap[0], 2]) and np.isfinite(r["coef"][gap[0], [1, 3]]).all() and r["df_h"][gap[0]] == 2
    assert (O.reference("n257", "additive", 12, maxit=2)["flags"] & O.MAXIT_BIT).any()
    kept = [O.analysis(c, "additive")[0].n for c in O.CASES]                        # three of each cohort have an unknown allele
    assert kept == [40, 255, 256, 257, 1000] and [-(-k // 128) * 128 for k in kept] == [128, 256, 256, 384, 1024]


def test_safety_conditions_of_the_device_tests():
    """In the restatement no convergence criterion of any compared fit lies within 1e-6 epsilon of epsilon, and every pivot
    ratio d_j / A_jj is below 1e-13 (aliased exactly) or above 1e-9 (well clear of the rule's 1e-11): so the device's
    iteration counts, dropped columns and degrees of freedom must equal the restatement's.  Measured: the closest criterion is
    5.6e-3 relative away; the ratios are at most 3.4e-14 in absolute value or at least 0.18."""
    logs = []
    for run in O.DEVICE_RUNS:
        for dtype in (np.float64, np.longdouble):
            r = O.reference(*run, dtype=dtype)
            logs.append((r["crit"], r["ratios"]))
    for model in ("additive", "dominant"):                                         # the one-row sets of the device tests
        A, covar, _, _ = O.analysis("n257", model)
        r = O.glm_sets(A.F, [[t] for t in range(A.n_tests)], covar[:12], None, A.y)
        logs.append((r["crit"], r["ratios"]))
    O.Backend.LOG.clear()                                                          # the end-to-end calls of the device tests
    hla, y, groups, covar = O.hla_of("n1000")
    for kw in ({}, {"condition": ["p3"]}, {"model": "dominant", "use_prob": True, "condition": ["p2", "03:01"]}):
        hb.hlaAssocOmnibus(hla, y, groups, covar[:, :6], _backend=O.Backend, **kw)
    hb.hlaAssocStepwise(hla, y, O.hla_of("n1000", without=("p3b",))[2], covar[:, :6], p_stop=1e-6, _backend=O.Backend)
    logs += O.Backend.LOG
    crit = np.array([c for cs, _ in logs for f in cs for c in f])
    ratios = np.array([v for _, rs in logs for f in rs for v in f])
    assert len(crit) > 500 and len(ratios) > 5000
    closest = float(np.min(np.abs(crit / 1e-8 - 1)))
    small = np.abs(ratios[ratios <= 1e-9])
    print(f"closest criterion {closest:.3g} relative; {len(small)} aliased pivots at most {small.max():.3g}, the others at least {ratios[ratios > 1e-9].min():.3g}")
    assert closest > 1e-6
    assert len(small) >= 10 and (small < 1e-13).all() and ratios[ratios > 1e-9].min() > 1e-9


def test_exports():
    for name in ("hibag_hip_assoc_glm_sets", "hibag_hip_assoc_row_sums"):
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    assert "int hibag_hip_assoc_glm_sets(" in hdr and "int hibag_hip_assoc_row_sums(" in hdr
    assert "#define HIBAG_HIP_GLM_WIDE_SLOTS 32" in hdr and assocomni.SLOTS == O.SLOTS == 32
    assert (assocomni.FLAG_ALIASED, assocomni.FLAG_TOO_WIDE) == (O.ALIASED_BIT, O.TOO_WIDE_BIT) == (8, 16)
    for name in ("hlaAssocOmnibus", "hlaAssocStepwise", "HlaAssocOmnibusResult", "HlaAssocStepwiseResult"):
        assert name in hb.__all__ and getattr(hb, name) is getattr(assocomni, name)
