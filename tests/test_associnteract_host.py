"""hlaAssocInteract on the host: the restatement of DESIGN.md section 27 (tests/associnteract_reference.py) against section 23's
fit on the same plain columns, against an independent scipy.optimize maximum of the likelihood for fits with a product
column, and with exactly aliased products; hlaAssocInteract's own host side driven by the restatement in place of the
device; what the device runs cover; and the safety conditions of the device tests."""

import math
import os
import sys

import numpy as np
import pytest
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assocglm_reference as G  # noqa: E402
import associnteract_reference as I  # noqa: E402
import assocomni_reference as O  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, associnteract  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = I.UNUSED


def interact(case, q=6, **kw):
    hla, y, groups, covar = I.hla_of(case)
    return hb.hlaAssocInteract(hla, y, covar[:, :q] if q else None, groups=groups, _backend=I.Backend, **kw)


def design(case, model, terms, q):
    """X = [1 | the terms' columns | the first q covariates], y, the weights 1."""
    A, covar, _, _ = I.analysis(case, model)
    X = np.stack([np.ones(A.n)] + [I.term_column(A.F, a, b).astype(float) for a, b in terms] + list(covar[:q]), axis=1)
    return X, A.y.astype(float), np.ones(A.n)


# 1 the fit -------------------------------------------------------------------------------------------------------
def test_plain_terms_are_the_fit_of_section_23():
    """One and two plain terms through tests/assocglm_reference.py on the same columns: the slots of the covariates and the
    factorisation order differ (the terms after the covariates here), nothing else: 1e-12."""
    seen = 0
    for case, model, q in (("n257", "additive", 11), ("n1000", "dominant", 6), ("n40", "additive", 0)):
        A, covar, _, _ = I.analysis(case, model)
        ts = [t for t in range(I.CASES[case][1]) if A.rsum[t] >= 5]
        recs = [[(t, -1), U, U] for t in ts] + [[U, (ts[0], -1), (t, -1)] for t in ts[1:]]
        r = I.glm_terms(A.F, np.array(recs, np.int32), covar[:q], None, A.y)
        for f, rec in enumerate(recs):
            used = [(j, a) for j, (a, _) in enumerate(rec) if a >= 0]
            X, y, w = design(case, model, [(a, -1) for _, a in used], q)
            want = G.fit(X, y, w)
            slots = [0] + [1 + j for j, _ in used] + list(range(I.COV0, I.COV0 + q))
            assert r["flags"][f] == want["flags"] == 0 and r["iterations"][f] == want["iterations"] and r["df_h"][f] == len(used)
            scale = np.fmax(np.abs(want["coef"]), want["se"])
            assert (np.abs(r["coef"][f, slots] - want["coef"]) <= 1e-12 * scale).all()
            assert np.allclose(r["se"][f, slots], want["se"], rtol=1e-12, atol=0) and abs(r["deviance"][f] / want["deviance"] - 1) <= 1e-12
            assert np.isnan(np.delete(r["coef"][f], slots)).all() and np.isnan(np.delete(r["se"][f], slots)).all()
            seen += 1
    assert seen >= 30


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
    """The main and the full fit of the pairs of the four most frequent alleles, and of the levels 0 of p2 and p3, in the
    1000- and 256-sample cohorts (fits without a flag, of at most 8 iterations): both deviances and the likelihood-ratio
    statistic within 1e-8 relative (of the statistic itself, as tests/test_assocomni_host.py holds it), se within 5e-3
    (section 23 item 5: the weights of the last solve).  Measured: deviance 4.4e-16, LRT 4.9e-12 (a statistic of 0.093), se
    6.3e-6, est 9.6e-11 (units of max(|est|, se)) over 13 pairs."""
    worst = [0.0, 0.0, 0.0, 0.0]
    seen = 0
    for case, q in (("n1000", 6), ("n256", 5)):
        A, covar, _, part_rows = I.analysis(case, "additive")
        pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(part_rows[0][0], part_rows[1][0])]
        r = I.glm_terms(A.F, np.array([rec for a, b in pairs for rec in (I.main(a, b), I.full(a, b))], np.int32), covar[:q], None, A.y)
        for i, (a, b) in enumerate(pairs):
            if r["flags"][2 * i] != 0 or r["flags"][2 * i + 1] != 0 or r["iterations"][2 * i + 1] > 8:
                continue
            _, _, dev_m = _mle(design(case, "additive", [(a, -1), (b, -1)], q)[0], A.y.astype(float))
            bf, sef, dev_f = _mle(design(case, "additive", [(a, -1), (b, -1), (a, b)], q)[0], A.y.astype(float))
            slots = [0, 1, 2, 3] + list(range(I.COV0, I.COV0 + q))
            lrt, want_lrt = r["deviance"][2 * i] - r["deviance"][2 * i + 1], dev_m - dev_f
            gaps = [max(abs(r["deviance"][2 * i] / dev_m - 1), abs(r["deviance"][2 * i + 1] / dev_f - 1)), abs(lrt / want_lrt - 1),
                    float(np.max(np.abs(r["se"][2 * i + 1, slots] / sef - 1))),
                    float(np.max(np.abs(r["coef"][2 * i + 1, slots] - bf) / np.fmax(np.abs(bf), sef)))]
            worst = [max(x, g) for x, g in zip(worst, gaps)]
            assert gaps[0] <= 1e-8 and gaps[1] <= 1e-8 and gaps[2] <= 5e-3 and gaps[3] <= 1e-5, (case, a, b, gaps)
            assert r["df_h"][2 * i] == 2 and r["df_h"][2 * i + 1] == 3
            seen += 1
    assert seen >= 8
    print(f"independent maximum: deviance {worst[0]:.3g}, LRT {worst[1]:.3g}, se {worst[2]:.3g}, est {worst[3]:.3g} over {seen} pairs")


# 2 aliased columns -----------------------------------------------------------------------------------------------
def assert_equals_fit_without(res, f, terms, kept, case, model, q):
    """Fit f of res (terms as given, those at the indices ``kept`` still in it) is the fit on the kept terms alone."""
    X, y, w = design(case, model, [terms[j] for j in kept], q)
    want = O.fit(X, len(kept), y, w)
    slots = [0] + [1 + j for j in kept] + list(range(I.COV0, I.COV0 + q))
    assert want["flags"] == 0 and res["flags"][f] == I.ALIASED_BIT and res["iterations"][f] == want["iterations"]
    assert res["df_h"][f] == len(kept) and np.isnan(np.delete(res["coef"][f], slots)).all() and np.isnan(np.delete(res["se"][f], slots)).all()
    assert np.allclose(res["coef"][f, slots], want["coef"], rtol=1e-10, atol=1e-13) and np.allclose(res["se"][f, slots], want["se"], rtol=1e-10, atol=0)
    assert abs(res["deviance"][f] / want["deviance"] - 1) <= 1e-12


def test_a_product_equal_to_one_of_its_factors_is_dropped():
    """dominant: carrier of allele 0 times carrier of the level of p2 that holds allele 0 IS carrier of allele 0; the factors
    come first in the factorisation, so the product is the aliased one -- by the pivot rule, not by a sum."""
    case, model, q = "n1000", "dominant", 6
    A, covar, _, part_rows = I.analysis(case, model)
    lv = part_rows[0][0]
    assert np.array_equal(I.term_column(A.F, 0, lv), A.F[0])
    terms = I.full(0, lv)
    r = I.glm_terms(A.F, np.array([I.main(0, lv), terms], np.int32), covar[:q], None, A.y)
    assert r["flags"][0] == 0 and r["df_h"].tolist() == [2, 2, 0]
    assert_equals_fit_without(r, 1, terms, [0, 1], case, model, q)
    assert np.allclose(r["coef"][1, :3], r["coef"][0, :3], rtol=1e-10, atol=1e-13) and abs(r["deviance"][1] / r["deviance"][0] - 1) <= 1e-12
    assert min(abs(v) for v in r["ratios"][1]) < 1e-13


def test_a_product_nobody_carries_and_alleles_that_never_meet():
    """recessive: nobody is homozygous for two alleles, so every product of two alleles sums to 0 -- left out before the fit
    from the integer sum (bit 3); alone in a record it leaves nothing to fit (bit 1)."""
    case, model, q = "n257", "recessive", 3
    A, covar, _, _ = I.analysis(case, model)
    assert A.rsum[0] > 0 and A.rsum[1] > 0 and int(I.row_gram(A.F, 0, 2)[0, 1]) == 0
    terms = I.full(0, 1)
    r = I.glm_terms(A.F, np.array([terms, [(0, 1), U, U], [U] * 3], np.int32), covar[:q], None, A.y)
    assert_equals_fit_without(r, 0, terms, [0, 1], case, model, q)
    assert r["flags"][1:3].tolist() == [I.RANK_BIT, I.RANK_BIT] and r["df_h"][1:3].tolist() == [0, 0] and r["iterations"][1] == 0
    assert np.isnan(r["coef"][1:3]).all() and np.isnan(r["deviance"][1:3]).all() and not r["ratios"][1]
    # through hlaAssocInteract: such a pair is below min_both = 1 and is not submitted; with min_both = 0 it is, and has no test
    hla, y, groups, covar = I.hla_of(case)
    pair = [("01:01", "02:01")]
    off = hb.hlaAssocInteract(hla, y, covar[:, :q], model=model, pairs=pair, _backend=I.Backend)
    assert off.both[0] == 0 and off.flags_main[0] == off.flags_full[0] == I.RANK_BIT and np.isnan(off.lrt_p[0]) and np.isnan(off.est).all()
    on = hb.hlaAssocInteract(hla, y, covar[:, :q], model=model, pairs=pair, min_both=0, _backend=I.Backend)
    assert on.flags_main[0] == 0 and on.flags_full[0] == I.ALIASED_BIT and (on.df_main[0], on.df_full[0]) == (2, 2)
    assert np.isnan(on.lrt_p[0]) and np.isnan(on.est[0, 2]) and np.isfinite(on.est[0, :2]).all()
    assert np.array_equal(on.est[0, :2], r["coef"][0, 1:3]) and on.deviance_full[0] == on.deviance_main[0] and on.lrt_stat[0] == 0.0


def test_a_term_conditioned_on_is_dropped():
    """The conditioned column stands among the covariates, which come first: the pair's own column of it is the aliased one,
    in the main and in the full fit; the product stays, so the test stays."""
    r = interact("n1000", pairs=[("01:01", "02:01"), ("02:01", "03:01")], condition=["01:01"])
    plain = interact("n1000", pairs=[("02:01", "03:01")], condition=["01:01"])
    assert r.base["name"][-1] == "h[01:01]" and r.base["flags"] == 0
    assert r.flags_main[0] == r.flags_full[0] == I.ALIASED_BIT and (r.df_main[0], r.df_full[0]) == (1, 2)
    assert np.isnan(r.est[0, 0]) and np.isnan(r.se[0, 0]) and np.isfinite(r.est[0, 1:]).all() and np.isfinite(r.lrt_p[0])
    assert r.flags_full[1] == 0 and r.lrt_p[1] == plain.lrt_p[0] and np.array_equal(r.est[1], plain.est[0])
    # the remaining coefficients are those of the fit without the column
    A, covar, _, _ = I.analysis("n1000", "additive")
    cov = np.concatenate([covar[:6], A.F[[0]].astype(float)])
    res = I.glm_terms(A.F, np.array([I.full(0, 1), [U, (1, -1), (0, 1)]], np.int32), cov, None, A.y)
    assert res["flags"][:2].tolist() == [I.ALIASED_BIT, 0] and res["df_h"][:2].tolist() == [2, 2] and np.isnan(res["coef"][0, 1])
    assert np.allclose(res["coef"][0, 2:11], res["coef"][1, 2:11], rtol=1e-10, atol=1e-13) and abs(res["deviance"][0] / res["deviance"][1] - 1) <= 1e-12
    assert np.allclose(r.est[0, 1:], res["coef"][0, 2:4], rtol=0, atol=0)


# 3 hlaAssocInteract on the restatement -------------------------------------------------------------------------------
def test_default_pairs_their_order_and_columns():
    r = interact("n257", q=5)
    A, covar, _, _ = I.analysis("n257", "additive")
    names = G.allele_names(12)
    want_pairs = [(a, b) for a in range(12) for b in range(a + 1, 12)]
    assert (A.rsum[:12] > 0).all() and list(zip(r.name_a, r.name_b)) == [(names[a], names[b]) for a, b in want_pairs]
    assert r.model == "additive" and r.locus == "DRB1" and "66 pairs, 5 covariates" in repr(r)
    gram = I.row_gram(A.F, 0, 12)
    assert np.array_equal(r.both, [gram[a, b] for a, b in want_pairs]) and (r.both == 0).sum() >= 3
    sub = [p for p in range(66) if r.both[p] >= 1]
    want = I.glm_terms(A.F, np.array([rec for p in sub for rec in (I.main(*want_pairs[p]), I.full(*want_pairs[p]))], np.int32), covar[:5], None, A.y)
    for i, p in enumerate(sub):
        assert np.array_equal(r.est[p], want["coef"][2 * i + 1, 1:4], equal_nan=True) and np.array_equal(r.se[p], want["se"][2 * i + 1, 1:4], equal_nan=True)
        assert r.deviance_main[p] == want["deviance"][2 * i] and r.deviance_full[p] == want["deviance"][2 * i + 1]
        assert (r.flags_main[p], r.flags_full[p]) == (want["flags"][2 * i], want["flags"][2 * i + 1])
        assert (r.iterations_main[p], r.iterations_full[p]) == (want["iterations"][2 * i], want["iterations"][2 * i + 1])
        if r.flags_main[p] == 0 and r.flags_full[p] == 0:
            assert (r.df_main[p], r.df_full[p]) == (2, 3) and r.lrt_stat[p] == r.deviance_main[p] - r.deviance_full[p]
            assert r.lrt_p[p] == math.erfc(math.sqrt(max(r.lrt_stat[p], 0.0) / 2.0))
            z = r.est[p] / r.se[p]
            assert np.allclose(r.pval[p], [math.erfc(abs(v) / math.sqrt(2)) for v in z], rtol=1e-14)
            assert np.allclose(r.lower[p], r.est[p] - 1.959963984540054 * r.se[p]) and np.allclose(r.upper[p], r.est[p] + 1.959963984540054 * r.se[p])
    for p in range(66):
        if r.both[p] == 0:
            assert r.flags_main[p] == r.flags_full[p] == I.RANK_BIT and r.iterations_full[p] == 0 and np.isnan(r.lrt_p[p])
            assert np.isnan(r.est[p]).all() and np.isnan(r.deviance_main[p]) and np.isnan(r.lrt_stat[p])
    assert r.base["name"] == ["(Intercept)"] + [f"c{j + 1}" for j in range(5)] and r.base["flags"] == 0
    assert np.array_equal(r.base["est"], want["coef"][-1, [0, 4, 5, 6, 7, 8]]) and r.base["deviance"] == want["deviance"][-1]
    assert set(r.to_table()) == {"both", "lrt.st", "lrt.p"} | {f"{t}.{c}" for t in ("a", "b", "a:b") for c in ("est", "2.5%", "97.5%", "pval")}
    # partition levels are not among the default pairs
    hla, y, groups, cv = I.hla_of("n257")
    assert len(hb.hlaAssocInteract(hla, y, cv[:, :5], _backend=I.Backend).both) == 66


def test_explicit_pairs_min_both_weights_models_and_maxit():
    case, q, kw = I.END_TO_END[1]
    r = interact(case, q=q, **kw)
    assert r.name_a[2] == "p2:p2.0" and r.name_b[2] == "p3:p3.0" and r.model == "dominant" and len(r.both) == 7
    A, _, _, part_rows = I.analysis(case, "dominant")
    assert r.both[2] == int(A.F[part_rows[0][0]] @ A.F[part_rows[1][0]]) and r.both[6] == 0
    assert r.flags_full[5] == I.ALIASED_BIT and np.isnan(r.lrt_p[5]) and np.isnan(r.est[5, 2])          # 01:01 x p2.0 is 01:01
    assert r.flags_full[6] == I.RANK_BIT and r.base["name"][-1] == "h[03:01]"
    assert r.flags_main[1] == I.ALIASED_BIT and np.isnan(r.est[1, 0])                                 # 03:01 is conditioned on
    unweighted = interact(case, q=q, **{**kw, "use_prob": False})
    assert not np.array_equal(unweighted.est[0], r.est[0]) and np.array_equal(unweighted.both, r.both)
    strict = interact(case, q=q, **{**kw, "min_both": 17})
    assert strict.flags_full.tolist()[:2] == [I.RANK_BIT, I.ALIASED_BIT] and strict.both[0] == 16 and np.array_equal(strict.est[1], r.est[1], equal_nan=True)
    or_ = interact(case, q=q, show_or=True, **kw)
    assert np.allclose(or_.est, np.exp(r.est), equal_nan=True) and np.array_equal(or_.se, r.se, equal_nan=True) and "a:b.est_OR" in or_.to_table()
    for model in ("additive", "recessive"):
        m = interact(case, q=q, **{**kw, "model": model})
        assert m.model == model and np.isfinite(m.lrt_p[2])
    r2 = interact("n257", q=5, maxit=2)
    fitted = r2.both >= 1
    assert (r2.flags_full[fitted] & I.MAXIT_BIT).all() and np.isnan(r2.lrt_p).all() and np.isfinite(r2.est[fitted][:, :2]).all()
    assert (r2.iterations_full[fitted] == 2).all() and np.isfinite(r2.deviance_full[fitted]).all()
    hla, y, groups, covar = I.hla_of("n257")
    keep = np.asarray(hla.prob) >= 0.5
    r = hb.hlaAssocInteract(hla, y, {"age": covar[:, 0], "sex": covar[:, 1]}, prob_threshold=0.5, _backend=I.Backend)
    assert r.n_excluded == int((~keep).sum()) and r.base["name"] == ["(Intercept)", "age", "sex"]


def test_both_of_rows_further_apart_than_one_gram_call(monkeypatch):
    """Rows that one hibag_hip_assoc_row_gram call does not span: the same integers from the two rows themselves."""
    pairs = [("01:01", "12:01"), ("02:01", "p3:p3.1"), ("01:01", "02:01")]
    want = interact("n257", q=5, pairs=pairs)
    monkeypatch.setattr(associnteract, "MAX_GRAM_ROWS", 4)
    got = interact("n257", q=5, pairs=pairs)
    assert np.array_equal(got.both, want.both) and got.both.dtype == np.int64 and np.array_equal(got.est, want.est, equal_nan=True)


def test_the_planted_interaction_has_the_smallest_p():
    hla, y, covar, names = I.planted()
    r = hb.hlaAssocInteract(hla, y, covar, _backend=I.Backend)
    i = int(np.nanargmin(r.lrt_p))
    assert (r.name_a[i], r.name_b[i]) == (names[1], names[2]) and r.lrt_p[i] < 1e-8 and r.est[i, 2] > 1.0
    assert np.sort(r.lrt_p[np.isfinite(r.lrt_p)])[1] > 1e-4


def test_value_errors():
    hla, y, groups, covar = I.hla_of("n257")
    run = lambda *a, **kw: hb.hlaAssocInteract(hla, y, *a, _backend=I.Backend, **kw)          # noqa: E731
    with pytest.raises(ValueError, match="genotype"):
        run(model="genotype")
    with pytest.raises(ValueError, match="should be one of"):
        run(model="allelic")
    with pytest.raises(TypeError, match="HlaAlleleGroups"):
        run(groups=3)
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="maxit"):
            run(maxit=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            run(epsilon=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_both"):
            run(min_both=bad)
    c = covar[:, :2].copy()
    c[7, 1] = np.nan
    with pytest.raises(ValueError, match="'c2' has a missing"):
        run(c)
    with pytest.raises(ValueError, match="has 5 values"):
        run(np.zeros((5, 1)))
    with pytest.raises(ValueError, match="list of test names"):
        run(condition=[3])
    with pytest.raises(ValueError, match="'p9' is not a test"):
        run(condition=["p9"])
    with pytest.raises(ValueError, match="condition: no allele of the data"):
        run(groups=groups, condition=["p2:p2.beyond"])
    with pytest.raises(ValueError, match=r"12 covariate columns \(2 conditioned"):
        run(covar[:, :10], condition=["01:01", "02:01"])
    assert len(run(covar[:, :10], condition=["01:01"], pairs=[("02:01", "03:01")]).base["name"]) == 12     # 11 columns are fine
    with pytest.raises(ValueError, match="pairs: 'p3:p3.1' is not a test"):
        run(pairs=[("01:01", "p3:p3.1")])                                                    # (a level, without groups)
    with pytest.raises(ValueError, match="pairs: '99:01' is not a test"):
        run(groups=groups, pairs=[("01:01", "02:01"), ("99:01", "01:01")])
    with pytest.raises(ValueError, match="pairs: no allele of the data belongs to 'p2:p2.beyond'"):
        run(groups=groups, pairs=[("01:01", "p2:p2.beyond")])
    with pytest.raises(ValueError, match="paired with itself"):
        run(pairs=[("02:01", "02:01")])
    for bad in (["01:01", "02:01"], [("01:01",)], [("01:01", "02:01", "03:01")], [("01:01", 2)], ["0102"]):
        with pytest.raises(ValueError, match=r"list of \(name, name\)"):
            run(pairs=bad)
    twice = np.column_stack([covar[:, :3], covar[:, 1]])
    with pytest.raises(ValueError, match="collinear"):
        run(twice, pairs=[("01:01", "02:01")])
    no_prob = hb.HlaAlleleClass(locus="A", sample_id=hla.sample_id, allele1=hla.allele1, allele2=hla.allele2)
    with pytest.raises(ValueError, match="No posterior probability"):
        hb.hlaAssocInteract(no_prob, y, use_prob=True, _backend=I.Backend)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocInteract(hla, y[:-1], _backend=I.Backend)
    assert len(run(pairs=[]).both) == 0 and run(pairs=[]).base["flags"] == 0


# 4 what the device tests rest on ---------------------------------------------------------------------------------
def test_the_device_runs_cover_the_shapes():
    """Read off the restatement: the three models, maxit = 2, prior weights, q = 0 and q = 11, fits of 1, 2 and 3 terms, a
    product with sum 0 beside carried main effects, an exactly aliased product, a record with no term; in every run at least
    three fitted fits and an active product."""
    assert {r[1] for r in I.DEVICE_RUNS} == set(I.MODELS) and {r[2] for r in I.DEVICE_RUNS} >= {0, 1, 5, 6, 11}
    assert any(r[4] == 2 for r in I.DEVICE_RUNS) and any(r[3] and r[0] == "n257" for r in I.DEVICE_RUNS)
    assert [I.CASE_Q[c] for c in I.CASES] == [0, 1, 5, 11, 6]
    aliased_exactly = 0
    for run in I.DEVICE_RUNS:
        r, fits = I.reference(*run), I.run_fits(*run[:2])
        fitted = (r["flags"][:-1] & I.RANK_BIT) == 0
        assert fitted.sum() >= 3 and {int(d) for d in r["df_h"][:-1][fitted]} >= {1, 2, 3}
        product = fits[:, 2, 1] >= 0
        assert (product & fitted & np.isfinite(r["coef"][:-1, 3])).any()                      # an active product
        zero = [f for f in np.flatnonzero(product & fitted) if I.term_column(I.analysis(*run[:2])[0].F, *fits[f, 2]).sum() == 0]
        empty = [f for f in zero if fits[f, 1, 0] >= 0]                                        # beside two carried main effects
        assert empty and all(r["flags"][f] & I.ALIASED_BIT and r["df_h"][f] == 2 and np.isnan(r["coef"][f, 3]) for f in empty)
        assert np.isfinite(r["coef"][empty[0], 1:3]).all()
        f = int(np.flatnonzero((fits == -1).all(axis=(1, 2)))[0])
        assert r["flags"][f] == I.RANK_BIT and r["df_h"][f] == 0 and np.isnan(r["coef"][f]).all()
        dropped = [f for f in np.flatnonzero(product & fitted) if f not in zero and np.isnan(r["coef"][f, 3])]
        aliased_exactly += len(dropped)
        assert all(min(abs(v) for v in r["ratios"][f]) < 1e-13 and r["flags"][f] & I.ALIASED_BIT for f in dropped)
        if run[1] != "additive":
            assert dropped
    assert aliased_exactly >= 2
    assert (I.reference("n257", "additive", 11, maxit=2)["flags"] & I.MAXIT_BIT).any()
    r = I.reference("n1000", "additive", 6)
    assert r["flags"][-3] == I.ALIASED_BIT and r["df_h"][-3] == 1 and np.isnan(r["coef"][-3, 1]) and r["flags"][-2] == I.RANK_BIT
    kept = [I.analysis(c, "additive")[0].n for c in I.CASES]
    assert kept == [40, 255, 256, 257, 1000] and [-(-k // 128) * 128 for k in kept] == [128, 256, 256, 384, 1024]


def test_safety_conditions_of_the_device_tests():
    """In the restatement, in both precisions, no convergence criterion of any compared fit lies within 1e-6 epsilon of
    epsilon, and every pivot ratio d_j / A_jj is below 1e-13 in absolute value (aliased exactly) or above 1e-9 (well clear of
    the rule's 1e-11): so the device's iteration counts, dropped columns and degrees of freedom must equal the restatement's.
    Measured: the closest criterion is 1.9e-2 relative away; the aliased ratios are at most 1.4e-16, the others at least 0.056."""
    class LongBackend(I.Backend):
        dtype = np.longdouble

    logs = []
    for run in I.DEVICE_RUNS:
        for dtype in (np.float64, np.longdouble):
            r = I.reference(*run, dtype=dtype)
            logs.append((r["crit"], r["ratios"]))
    for model in ("additive", "dominant"):                                         # the plain-term fits of the device tests
        A, covar, _, _ = I.analysis("n257", model)
        fits = np.array([[(t, -1), U, U] for t in range(A.n_tests)], np.int32)
        for dtype in (np.float64, np.longdouble):
            r = I.glm_terms(A.F, fits, covar[:11], None, A.y, dtype=dtype)
            logs.append((r["crit"], r["ratios"]))
    I.Backend.LOG.clear()                                                          # the end-to-end calls of the device tests
    for case, q, kw in I.END_TO_END:
        hla, y, groups, covar = I.hla_of(case)
        for backend in (I.Backend, LongBackend):
            hb.hlaAssocInteract(hla, y, covar[:, :q], groups=groups, _backend=backend, **kw)
    logs += I.Backend.LOG
    crit = np.array([c for cs, _ in logs for f in cs for c in f])
    ratios = np.array([v for _, rs in logs for f in rs for v in f])
    assert len(crit) > 500 and len(ratios) > 5000
    closest = float(np.min(np.abs(crit / 1e-8 - 1)))
    small = np.abs(ratios[ratios <= 1e-9])
    print(f"closest criterion {closest:.3g} relative; {len(small)} aliased pivots at most {small.max():.3g}, the others at least {ratios[ratios > 1e-9].min():.3g}")
    assert closest > 1e-6
    assert len(small) >= 4 and (small < 1e-13).all() and ratios[ratios > 1e-9].min() > 1e-9


def test_exports():
    for name in ("hibag_hip_assoc_glm_terms", "hibag_hip_assoc_row_gram"):
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    assert "int hibag_hip_assoc_glm_terms(" in hdr and "int hibag_hip_assoc_row_gram(" in hdr
    assert "#define HIBAG_HIP_GLM_TERMS_MAX_COVAR 11" in hdr and associnteract.MAX_COVAR == I.MAX_COVAR == 11
    assert (associnteract.SLOTS, associnteract.COV0, associnteract.TERMS) == (I.SLOTS, I.COV0, I.TERMS) == (16, 4, 3)
    assert associnteract.FLAG_ALIASED == I.ALIASED_BIT == 8
    for name in ("hlaAssocInteract", "HlaAssocInteractResult"):
        assert name in hb.__all__ and getattr(hb, name) is getattr(associnteract, name)
