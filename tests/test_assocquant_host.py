"""hlaAssocQuant on the host: the restatement of DESIGN.md section 25 (tests/assocquant_reference.py) against scipy's Welch
t-test and one-way ANOVA, against numpy's least squares on the full design and a brute-force Freedman-Lane refit; the
package's incomplete beta function against scipy's; the permutation generator; the NaN and rank rules; hlaAssocQuant's own
host side (condition, every ValueError) end to end on the restatement; and the safety condition of the GPU comparisons.

Bounds against scipy and lstsq: ten times the largest difference measured here, never looser than 1e-9 relative (the
measured values are in DESIGN.md section 25, "Checks", and printed by the tests)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_reference as AR  # noqa: E402
import assocquant_reference as Q  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assocquant  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured on the cases below -> the bound (10 x measured, at most 1e-9)
BOUND_TTEST = 3e-12        # measured 2.92e-13 (ttest_p against scipy.stats.ttest_ind(equal_var=False), relative)
BOUND_ANOVA = 7.5e-11      # measured 7.21e-12 (anova_p against scipy.stats.f_oneway, relative)
BOUND_LSTSQ = 3.5e-10      # measured 3.3e-11: est and se in units of max(|est|, se), F and rss relative
BOUND_LSTSQ_P = 1.2e-10    # measured 1.17e-11: the t-test and F p-values against scipy's tails at lstsq's statistics, relative
BOUND_BETAINC = 3.6e-10    # measured 3.53e-11 relative over the grid and the tails near 1e-300


def kept_case(case):
    n, n_allele, q, seed, n_na, part = Q.CASES[case]
    a1, a2, y, g, covar = Q.cohort(n, n_allele, q, seed, n_na, part)
    yk, ck = Q.kept_columns(a1, a2, y, covar)
    return a1, a2, yk, g, ck, n_allele


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]), initial=0.0))


# 1 the class columns against scipy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n40", "n257", "n1000"])
def test_class_columns_equal_scipy(case):
    stats = pytest.importorskip("scipy.stats")
    hla, y, groups, covar = Q.hla_of(case)
    a1, a2, yk, g, ck, n_allele = kept_case(case)
    worst_t = worst_f = 0.0
    seen = {m: 0 for m in Q.MODELS}
    for model in Q.MODELS:
        res = hb.hlaAssocQuant(hla, y, covar, model=model, groups=groups, _backend=Q.Backend)
        A = AR.Analysis(a1, a2, np.zeros(len(a1), np.int32), n_allele, g, model)
        cls = A.F[0::2] + 2 * A.F[1::2] if model == "genotype" else A.F
        for t, row in enumerate(res.name):
            if t >= len(cls):            # (a level the device does not know: NaN)
                continue
            parts = [yk[cls[t] == k] for k in range(3)]
            for k in range(res.avg.shape[1]):
                assert res.counts[t, k] == len(parts[k])
                if len(parts[k]):
                    assert abs(res.avg[t, k] - parts[k].mean()) <= 1e-12 * abs(parts[k].mean())
                else:
                    assert math.isnan(res.avg[t, k])
            if model in ("dominant", "recessive"):
                assert res.anova_p is None
                if min(len(parts[0]), len(parts[1])) < 2:
                    assert math.isnan(res.ttest_p[t])
                    continue
                want = stats.ttest_ind(parts[0], parts[1], equal_var=False).pvalue
                worst_t = max(worst_t, abs(res.ttest_p[t] / want - 1))
            else:
                assert res.ttest_p is None
                full = [p for p in parts if len(p)]
                if len(full) < 2:
                    assert math.isnan(res.anova_p[t])
                    continue
                want = stats.f_oneway(*full).pvalue
                worst_f = max(worst_f, abs(res.anova_p[t] / want - 1))
            seen[model] += 1
    assert min(seen.values()) >= (3 if case != "n40" else 0) and seen["dominant"] >= 3 and seen["genotype"] >= 3, seen
    print(f"{case}: ttest_p within {worst_t:.3g} of scipy, anova_p within {worst_f:.3g}")
    assert worst_t <= BOUND_TTEST and worst_f <= BOUND_ANOVA


# 2 the regression columns against least squares on the full design -----------------------------------------------------
def lstsq_fit(yk, ck, cols):
    n = len(yk)
    X = np.column_stack([np.ones(n)] + list(ck) + cols)
    beta = np.linalg.lstsq(X, yk, rcond=None)[0]
    r = yk - X @ beta
    df = n - X.shape[1]
    s2 = (r @ r) / df
    cov = s2 * np.linalg.inv(X.T @ X)
    d = len(cols)
    F = beta[-d:] @ np.linalg.solve(cov[-d:, -d:], beta[-d:]) / d       # (the Wald form: no difference of two sums of squares)
    return beta[-d:], np.sqrt(np.diag(cov)[-d:]), F, df, r @ r


@pytest.mark.parametrize("case", ["n40", "n256", "n257", "n1000"])
def test_regression_columns_equal_lstsq(case):
    hla, y, groups, covar = Q.hla_of(case)
    a1, a2, yk, g, ck, n_allele = kept_case(case)
    worst = worst_p = 0.0
    try:
        from scipy import stats
    except ImportError:
        stats = None
    for model in Q.MODELS:
        res = hb.hlaAssocQuant(hla, y, covar, model=model, groups=groups, _backend=Q.Backend)
        A = AR.Analysis(a1, a2, np.zeros(len(a1), np.int32), n_allele, g, model)
        seen = 0
        for t in range(A.n_tests):
            if res.flags[t] & 2:
                assert np.isnan(res.est[t]).all() and math.isnan(res.stat[t])
                continue
            rows = [2 * t, 2 * t + 1] if model == "genotype" else [t]
            used = [j for j, r in enumerate(rows) if A.F[r].any()]
            est, se, F, df, rss = lstsq_fit(yk, ck, [A.F[rows[j]].astype(np.float64) for j in used])
            assert df == res.df[t]
            scale = np.fmax(np.abs(est), se)
            worst = max(worst, np.max(np.abs(res.est[t, used] - est) / scale), np.max(np.abs(res.se[t, used] - se) / scale),
                        abs(res.stat[t] / F - 1) if F > 1e-6 else 0.0, abs(res.rss[t] / rss - 1))
            unused = [j for j in range(len(rows)) if j not in used]
            assert np.isnan(res.est[t, unused]).all() and np.isnan(res.pval[t, unused]).all()
            assert np.allclose(res.lower[t, used], res.est[t, used] - 1.959963984540054 * res.se[t, used], rtol=1e-15, atol=0)
            assert np.allclose(res.upper[t, used], res.est[t, used] + 1.959963984540054 * res.se[t, used], rtol=1e-15, atol=0)
            if stats is not None:
                want_p = 2 * stats.t.sf(np.abs(est / se), df)
                worst_p = max(worst_p, np.max(np.abs(res.pval[t, used] / want_p - 1)),
                              abs(res.stat_p[t] / stats.f.sf(F, len(used), df) - 1))
            seen += 1
        assert seen >= 3
    print(f"{case}: est, se, F, rss within {worst:.3g} of lstsq; p-values within {worst_p:.3g} of scipy's tails")
    assert worst <= BOUND_LSTSQ and worst_p <= BOUND_LSTSQ_P


# 3 the incomplete beta function -------------------------------------------------------------------------------------------
def test_betainc_equals_scipy_on_a_grid():
    special = pytest.importorskip("scipy.special")
    ab = [0.5, 1.0, 1.5, 2.0, 3.5, 10.0, 49.5, 100.0, 498.5, 1000.0, 2500.0, 5000.0]
    worst, n = 0.0, 0
    for a in ab:
        for b in ab:
            xs = [1e-300, 1e-200, 1e-100, 1e-30, 1e-10, 1e-4, 0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 1 - 1e-6, 1 - 1e-12]
            mid = a / (a + b)
            xs += [mid * f for f in (0.25, 0.5, 0.8, 0.95, 1.0, 1.05, 1.25, 2.0) if mid * f < 1]
            for x in xs:
                want = float(special.betainc(a, b, x))
                got = assocquant.betainc(a, b, x)
                if want < 1e-300:                # the tail underflows in both
                    assert got < 1e-290, (a, b, x, got)
                    continue
                worst = max(worst, abs(got / want - 1))
                n += 1
    print(f"betainc: {n} points, within {worst:.3g} relative of scipy.special.betainc")
    assert n > 2000 and worst <= BOUND_BETAINC
    # tails of 1e-300 themselves: x with I_x(a, b) ~ x^a / (a B(a, b)) = 1e-300
    tails = 0
    for a in (1.0, 1.5, 10.0, 500.0, 5000.0):
        for b in (0.5, 1.0, 3.5):
            x = math.exp((math.log(1e-300) + math.log(a) + math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)) / a)
            want = float(special.betainc(a, b, x))
            assert 1e-305 < want < 1e-250, (a, b, x, want)
            worst = max(worst, abs(assocquant.betainc(a, b, x) / want - 1))
            tails += 1
    print(f"betainc: with {tails} tails near 1e-300, within {worst:.3g}")
    assert worst <= BOUND_BETAINC
    assert assocquant.betainc(2.0, 3.0, 0.0) == 0.0 and assocquant.betainc(2.0, 3.0, 1.0) == 1.0
    assert math.isnan(assocquant.betainc(2.0, 3.0, math.nan))


def test_betainc_closed_forms():
    """Without scipy: I_x(1, b) = 1 - (1 - x)^b, I_x(a, 1) = x^a, I_x(1/2, 1/2) = (2 / pi) asin sqrt x, and the reflection."""
    for x in (1e-9, 0.01, 0.3, 0.5, 0.77, 0.999):
        for b in (0.5, 2.0, 17.0, 300.0):
            assert abs(assocquant.betainc(1.0, b, x) - (-math.expm1(b * math.log1p(-x)))) <= 1e-12 * (-math.expm1(b * math.log1p(-x)))
            assert abs(assocquant.betainc(b, 1.0, x) - x ** b) <= 1e-12 * x ** b
            assert abs(assocquant.betainc(b, 3.5, x) + assocquant.betainc(3.5, b, 1 - x) - 1) <= 1e-12
        assert abs(assocquant.betainc(0.5, 0.5, x) - 2 / math.pi * math.asin(math.sqrt(x))) <= 1e-12


# 4 Freedman-Lane against a brute-force refit ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", Q.MODELS)
def test_freedman_lane_identity(model):
    """T of items 6-7 = the t^2 / F of a full least-squares refit of y* = fitted + permuted residuals on [Z, x]."""
    a1, a2, yk, g, ck, n_allele = kept_case("n256")
    A = AR.Analysis(a1, a2, np.zeros(len(a1), np.int32), n_allele, g, model)
    Z = Q.Quant(A.F, model, yk, ck)
    n = Z.n
    X0 = np.column_stack([np.ones(n)] + list(ck))
    fitted = X0 @ np.linalg.lstsq(X0, yk, rcond=None)[0]
    resid = yk - fitted
    assert np.max(np.abs(resid - Z.yt)) <= 1e-10 * np.max(np.abs(resid))
    perms = Q.perm_rows(5, 0, 6, n)                     # permutation 0, the observed run, among them
    T = Z.run(perms)[2]
    worst = 0.0
    for p in range(len(perms)):
        ystar = fitted + resid[perms[p]]
        for t in range(Z.T):
            if Z.tests[t] is None:
                continue
            cols = [A.F[r].astype(np.float64) for r in Z.tests[t][:2] if r >= 0]
            F = lstsq_fit(ystar, ck, cols)[2]
            worst = max(worst, abs(T[t, p] / F - 1) if F > 1e-3 else abs(T[t, p] - F))
    print(f"{model}: T within {worst:.3g} of the brute-force refit")
    assert worst <= 1e-9                   # (measured 4.1e-11; the refit's own conditioning is part of it)
    assert np.allclose(T[:, 0], Z.stat, rtol=1e-12, atol=0, equal_nan=True)          # permutation 0 is the observed run


# 5 the generator ------------------------------------------------------------------------------------------------------
def test_generator():
    n = 23
    rows = Q.perm_rows(0xDEADBEEFCAFEF00D, 1, 4000, n)
    assert rows.dtype == np.int32 and (np.sort(rows, axis=1) == np.arange(n)).all()          # every row a permutation
    # position frequencies: value v at position i in 4000 / n of the rows, binomial standard error
    freq = np.stack([(rows == v).sum(axis=0) for v in range(n)])
    p = 1.0 / n
    assert np.max(np.abs(freq - 4000 * p)) <= 5 * math.sqrt(4000 * p * (1 - p))
    assert len({r.tobytes() for r in rows}) == 4000
    # split ranges concatenate; a row depends on (seed, p, n) alone
    big = (1 << 63) + 12345
    whole = Q.perm_rows(7, big, 40, n)
    assert np.array_equal(np.concatenate([Q.perm_rows(7, big, 13, n), Q.perm_rows(7, big + 13, 27, n)]), whole)
    assert not np.array_equal(Q.perm_rows(8, big, 1, n), whole[:1]) and not np.array_equal(Q.perm_rows(7 + (1 << 32), big, 1, n), whole[:1])
    assert not np.array_equal(Q.perm_rows(7, big + (1 << 32), 1, n), whole[:1])
    assert np.array_equal(Q.perm_rows(7, 0, 1, n)[0], np.arange(n))                            # permutation 0: the identity
    # n = 5 by hand.  seed 0x0123456789ABCDEF, p = 2^40 + 7: Philox4x32-10(counter (0, 1, 7, 256), key (0x89ABCDEF, 0x01234567))
    # = (590131812, 2809323722, 165849785, 2126930213), counter (1, 1, 7, 256) starts with 12765974.
    #   i = 0: j = 0                                  -> [0]
    #   i = 1: 2809323722 * 2 >> 32 = 1               -> [0, 1]
    #   i = 2: 165849785 * 3 >> 32 = 0: row[2] = row[0] = 0, row[0] = 2  -> [2, 1, 0]
    #   i = 3: 2126930213 * 4 >> 32 = 1: row[3] = row[1] = 1, row[1] = 3 -> [2, 3, 0, 1]
    #   i = 4: 12765974 * 5 >> 32 = 0: row[4] = row[0] = 2, row[0] = 4   -> [4, 3, 0, 1, 2]
    from draws_reference import philox4x32_10
    w = philox4x32_10(np.array([[0, 1, 7, 256], [1, 1, 7, 256]], np.uint64), np.array([0x89ABCDEF, 0x01234567], np.uint64))
    assert w[0].tolist() == [590131812, 2809323722, 165849785, 2126930213] and int(w[1, 0]) == 12765974
    assert Q.perm_rows(0x0123456789ABCDEF, (1 << 40) + 7, 1, 5).tolist() == [[4, 3, 0, 1, 2]]
    # the stream is apart from hlaAssocTest's labels (counter word 1 = 0 there)
    assert not np.array_equal(philox4x32_10(np.array([0, 0, 7, 256], np.uint64), np.array([0x89ABCDEF, 0x01234567], np.uint64)), w[0])


# 6 item 4's NaN rules -------------------------------------------------------------------------------------------------
def test_class_nan_rules():
    f = assocquant._class_columns
    cnt = np.array([[5, 1, 0], [4, 2, 0], [0, 6, 0], [3, 3, 0]], np.int64)
    S1 = np.array([[1.0, -1.0, 0], [2.0, -2.0, 0], [0, 0.0, 0], [0.0, 0.0, 0]])
    S2 = np.array([[3.0, 1.0, 0], [4.0, 5.0, 0], [0, 7.0, 0], [0.0, 0.0, 0]])
    avg, tp, ap = f("dominant", cnt, S1, S2, 10.0, 6)
    assert ap is None and avg.shape == (4, 2)
    assert math.isnan(tp[0])                                   # a class with fewer than 2 samples
    assert 0 < tp[1] < 1
    assert math.isnan(tp[2]) and math.isnan(avg[2, 0]) and avg[2, 1] == 10.0     # an empty class
    assert math.isnan(tp[3])                                   # data essentially constant: se < 10 eps max |avg|
    cnt = np.array([[6, 0, 0], [3, 2, 1], [3, 0, 3], [1, 1, 1]], np.int64)
    S1 = np.array([[0.0, 0, 0], [1.0, 1.0, -2.0], [3.0, 0, -3.0], [1.0, 0.0, -1.0]])
    S2 = np.array([[5.0, 0, 0], [2.0, 3.0, 4.0], [4.0, 0, 5.0], [1.0, 0.0, 1.0]])
    avg, tp, ap = f("genotype", cnt, S1, S2, 0.0, 6)
    assert tp is None and avg.shape == (4, 3)
    assert math.isnan(ap[0])                                   # k < 2
    assert 0 < ap[1] < 1 and 0 < ap[2] < 1                     # three classes; two classes (the empty one left out)
    assert math.isnan(f("additive", cnt[3:], S1[3:], S2[3:], 0.0, 3)[2][0])      # n - k < 1


# 7 RANK for every kind of column ------------------------------------------------------------------------------------------
def test_rank_rules():
    n = 12
    y = np.arange(n, dtype=np.float64) ** 1.5
    c1 = np.array([0, 1] * 6, np.float64)

    def flags(F, model, covar=None):
        return Q.Quant(np.array(F, np.int64), model, y, covar).flags.tolist()

    one, zero = [1] * n, [0] * n
    half = [1] * 6 + [0] * 6
    assert flags([zero, one, half], "dominant") == [2, 2, 0]                       # constant columns
    assert flags([[2] * n, one, [2] * 6 + [1] * 6], "additive") == [2, 2, 0]           # all 2, all 1 (constant, not 0 or 2 n)
    assert flags([c1.astype(int).tolist(), half], "recessive", [c1]) == [2, 0]      # a column in the span of the covariates
    assert flags([(2 * c1).astype(int).tolist()], "additive", [c1]) == [2]
    het, hom = [1] * 4 + [0] * 8, [0] * 4 + [1] * 4 + [0] * 4
    Z = Q.Quant(np.array([het, hom, het, zero, zero, hom, zero, zero, het, [1 - v for v in het]], np.int64), "genotype", y)
    assert Z.flags.tolist() == [0, 0, 0, 2, 2]                                  # both, het alone, hom alone, nobody, nobody in class 0
    assert Z.tests[0][1] == 1 and Z.tests[1][:2] == (2, -1) and Z.tests[2][:2] == (5, -1)
    assert Z.tests[0][2] == n - 1 - 2 and Z.tests[1][2] == n - 1 - 1                # d = 1 for a dummy left out
    # a combination of the two dummies in the span of the covariates (det), one dummy in it (a11)
    hv, mv = np.array(het, np.float64), np.array(hom, np.float64)
    for cov, want in (([hv + 2 * mv, c1], [2]), ([hv - mv, c1], [2]), ([hv, c1], [2]), ([c1], [0])):
        Z = Q.Quant(np.array([het, hom], np.int64), "genotype", y, cov)
        assert Z.flags.tolist() == want and np.isnan(Z.stat).tolist() == [w == 2 for w in want]
    with pytest.raises(Q.Collinear):
        Q.Quant(np.array([half], np.int64), "dominant", y, [c1, 3 * c1 + 2])
    with pytest.raises(Q.Collinear):
        Q.Quant(np.array([half], np.int64), "dominant", y, [np.full(n, 4.0)])
    with pytest.raises(ValueError):
        Q.Quant(np.array([half[:3]], np.int64), "dominant", y[:3], [c1[:3]])        # df < 1


# 8 hlaAssocQuant's host side, on the restatement ----------------------------------------------------------------------
def test_end_to_end_on_the_restatement():
    hla, y, groups, covar = Q.hla_of("n1000")
    seed = Q.seed_of("n1000", "dominant")
    res = hb.hlaAssocQuant(hla, y, covar, groups=groups, n_perm=65, seed=seed, _backend=Q.Backend)
    Z = Q.reference("n1000", "dominant")
    assert res.name[:65] == Q.allele_names(65) and res.name[-1] == "pos:beyond" and len(res.name) == 70
    assert res.n_samp == 997 and res.n_excluded == 0 and res.n_perm == 65 and res.seed == seed
    assert res.covariates == [f"c{j + 1}" for j in range(6)] and res.h_names == ("h",)
    assert np.array_equal(res.stat[:69], Z.stat, equal_nan=True) and np.array_equal(res.flags[:69], Z.flags)
    assert res.flags[-1] == 2 and math.isnan(res.stat[-1]) and math.isnan(res.perm_p[-1]) and res.counts[-1].tolist() == [997, 0]
    assert abs(res.avg[-1, 0] - float(Z.ybar)) <= 1e-12 * abs(float(Z.ybar)) and math.isnan(res.avg[-1, 1])
    assert np.allclose(res.max_stat, Z.max_stat[:65], rtol=1e-12, atol=0)         # (a product of 65 columns and one of 200 round differently)
    with np.errstate(invalid="ignore"):
        count = (Z.perm_T[:, :65] >= Z.stat[:, None]).sum(axis=1)
        count_max = (Z.max_stat[None, :65] >= Z.stat[:, None]).sum(axis=1)
    fitted = Z.flags == 0
    assert np.array_equal(res.perm_p[:69][fitted], ((1 + count) / 66)[fitted])
    assert np.array_equal(res.perm_p_adj[:69][fitted], ((1 + count_max) / 66)[fitted])
    assert np.isnan(res.perm_p[:69][~fitted]).all() and (res.perm_p_adj[:69][fitted] >= res.perm_p[:69][fitted]).all()
    top = res.name[int(np.nanargmax(res.stat))]
    assert top in ("01:01", "02:01") and res.perm_p_adj[res.name.index(top)] == 1 / 66
    table = res.to_table()
    assert list(table)[:5] == ["[-/-]", "[-/h,h/h]", "avg.[-/-]", "avg.[-/h,h/h]", "ttest.p"]
    assert list(table)[5:] == ["h.est", "h.2.5%", "h.97.5%", "h.pval", "perm.p", "perm.p.adj"]
    assert "hlaAssocQuant" in hb.__all__ and "HlaAssocQuantResult" in hb.__all__ and "65 permutations" in repr(res)
    # a named dict of covariates, a drawn seed, the genotype model's columns, the call threshold
    named = {f"pc{j}": covar[:, j] for j in range(6)}
    gen = hb.hlaAssocQuant(hla, y, named, model="genotype", n_perm=3, _backend=Q.Backend)
    assert gen.covariates == list(named) and 0 <= gen.seed < 1 << 64 and gen.est.shape == (65, 2) and gen.h_names == ("h1", "h2")
    assert list(gen.to_table())[:7] == ["[-/-]", "[-/h]", "[h/h]", "avg.[-/-]", "avg.[-/h]", "avg.[h/h]", "anova.p"]
    hla.prob = np.linspace(0.2, 1.0, len(y))
    thr = hb.hlaAssocQuant(hla, y, covar, prob_threshold=0.5, _backend=Q.Backend)
    assert thr.n_excluded == int((hla.prob < 0.5).sum()) and thr.n_samp < 997
    assert hb.hlaAssocQuant(hla, y, _backend=Q.Backend).covariates == []


def test_condition():
    hla, y, groups, covar = Q.hla_of("n1000")
    res = hb.hlaAssocQuant(hla, y, covar, groups=groups, _backend=Q.Backend)
    top = res.name[int(np.nanargmax(res.stat))]
    seen = []

    class Recording(Q.Backend):
        def quant(self, yk, cov):
            seen.append(np.array(cov))
            return super().quant(yk, cov)

    cond = hb.hlaAssocQuant(hla, y, covar, groups=groups, condition=[top], _backend=Recording)
    i = res.name.index(top)
    a1, a2, yk, g, ck, n_allele = kept_case("n1000")
    A = AR.Analysis(a1, a2, np.zeros(len(a1), np.int32), n_allele, g, "dominant")
    assert seen[0].shape == (7, 997) and np.array_equal(seen[0][6], A.F[i]) and np.array_equal(seen[0][:6], ck)
    assert cond.covariates[-1] == f"h[{top}]" and cond.flags[i] == 2 and math.isnan(cond.stat[i])
    assert (cond.df[np.isfinite(cond.df)] == 997 - 1 - 7 - 1).all()
    j = (i + 1) % 65
    est = lstsq_fit(yk, list(ck) + [A.F[i].astype(np.float64)], [A.F[j].astype(np.float64)])[0]
    assert abs(cond.est[j, 0] - est[0]) <= 1e-9 * max(abs(est[0]), cond.se[j, 0])
    both = hb.hlaAssocQuant(hla, y, covar, model="genotype", groups=groups, condition=top, _backend=Q.Backend)
    assert both.covariates[-2:] == [f"h1[{top}]", f"h2[{top}]"] and both.flags[i] == 2


def test_value_errors():
    hla, y, groups, covar = Q.hla_of("n40")
    B = Q.Backend
    n = len(y)
    c = np.random.default_rng(0).standard_normal((n, 3))
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaAssocQuant(hla, y, model="dominent", _backend=B)
    with pytest.raises(ValueError, match="use_prob"):
        hb.hlaAssocQuant(hla, y, use_prob=True, _backend=B)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="n_perm"):
            hb.hlaAssocQuant(hla, y, n_perm=bad, _backend=B)
    for bad in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            hb.hlaAssocQuant(hla, y, n_perm=2, seed=bad, _backend=B)
    with pytest.raises(TypeError):
        hb.hlaAssocQuant("hla", y, _backend=B)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocQuant(hla, y[:-1], _backend=B)
    with pytest.raises(ValueError, match="numeric"):
        hb.hlaAssocQuant(hla, ["a"] * n, _backend=B)
    a1, a2 = Q.cohort(*Q.CASES["n40"])[:2]
    kept = np.flatnonzero((a1 >= 0) & (a2 >= 0))
    for v in (np.nan, np.inf):
        yy = y.copy()
        yy[kept[3]] = v
        with pytest.raises(ValueError, match="non-finite"):
            hb.hlaAssocQuant(hla, yy, _backend=B)
        cc = c.copy()
        cc[kept[5], 1] = v
        with pytest.raises(ValueError, match="'c2'"):
            hb.hlaAssocQuant(hla, y, cc, _backend=B)
    dropped = np.flatnonzero((a1 < 0) | (a2 < 0))
    yy = y.copy()
    yy[dropped[0]] = np.nan                                     # (a sample that is not kept may hold anything)
    assert hb.hlaAssocQuant(hla, yy, _backend=B).n_samp == 37
    with pytest.raises(ValueError, match="values for"):
        hb.hlaAssocQuant(hla, y, c[:-1], _backend=B)
    with pytest.raises(ValueError, match="array"):
        hb.hlaAssocQuant(hla, y, np.zeros((n, 1, 1)), _backend=B)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocQuant(hla, y, np.zeros((n, 13)), _backend=B)
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocQuant(hla, y, np.column_stack([c[:, 0], 2 * c[:, 0] + 1]), _backend=B)
    with pytest.raises(ValueError, match="not a test"):
        hb.hlaAssocQuant(hla, y, condition=["99:99"], _backend=B)
    with pytest.raises(ValueError, match="list of test names"):
        hb.hlaAssocQuant(hla, y, condition=[3], _backend=B)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocQuant(hla, y, np.random.default_rng(1).standard_normal((n, 12)), condition=["01:01"], _backend=B)
    small, ys, _, _ = Q.hla_of("n5")
    with pytest.raises(ValueError, match="degree of freedom"):
        hb.hlaAssocQuant(small, ys, np.random.default_rng(2).standard_normal((5, 2)), _backend=B)
    with pytest.raises(ValueError, match="degree of freedom"):
        hb.hlaAssocQuant(small, ys, np.random.default_rng(2).standard_normal((5, 1)), model="genotype", _backend=B)
    hlg, yg, grp, _ = Q.hla_of("n1000")
    with pytest.raises(ValueError, match="no allele of the data"):
        hb.hlaAssocQuant(hlg, yg, groups=grp, condition=["pos:beyond"], _backend=B)


# 9 the safety condition of the GPU comparisons ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", Q.MODELS)
@pytest.mark.parametrize("case", list(Q.CASES))
def test_no_permuted_statistic_near_the_observed_one(case, model):
    """Every |T[t][p] - T_obs[t]| of every case tests/test_hip_assocquant.py compares exceeds 1e-6 T_obs[t], so that the
    device's `>=` and the restatement's agree whatever the last bits; and the seed is the first that does."""
    Z = Q.reference(case, model)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.abs(Z.perm_T - Z.stat[:, None]) / Z.stat[:, None]
    assert Z.perm_T.shape[1] == Q.N_PERM[case] == max(Q.PERM_COUNTS[case]) and np.isfinite(gap).any()
    print(f"{case} {model}: closest gap {np.nanmin(gap):.3g}, tolerance {Q.tolerance(case, model):.3g}")
    assert np.nanmin(gap) > 1e-6
    for k in range(Q.SEEDS.get((case, model), 0)):
        assert Q.min_gap(Z, Q.PERM_SEED + k, Q.N_PERM[case]) <= 1e-6


def test_end_to_end_runs_meet_the_safety_condition():
    """The two hlaAssocQuant runs the GPU test compares: n1000 dominant, 65 permutations, plain and conditioned on the top hit."""
    hla, y, groups, covar = Q.hla_of("n1000")
    a1, a2, yk, g, ck, n_allele = kept_case("n1000")
    A = AR.Analysis(a1, a2, np.zeros(len(a1), np.int32), n_allele, g, "dominant")
    Z = Q.reference("n1000", "dominant")
    top = int(np.nanargmax(Z.stat))
    Zc = Q.Quant(A.F, "dominant", yk, np.concatenate([ck, A.F[top:top + 1].astype(np.float64)]))
    seed = Q.seed_of("n1000", "dominant")
    assert Q.min_gap(Zc, seed, 65) > 1e-6 and Q.min_gap(Z, seed, 65) > 1e-6
    # perm_p_adj compares every permutation's maximum with every observed statistic: those stay apart as well
    for z in (Z, Zc):
        best = np.nanmax(z.stats(seed, 1, 65), axis=0)
        with np.errstate(invalid="ignore"):
            assert np.nanmin(np.abs(best[None, :] - z.stat[:, None]) / z.stat[:, None]) > 1e-6


# 10 the interface ---------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    from hibag_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    declared = set(re.findall(r"\b(hibag_hip_assoc_quant_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"hibag_hip_assoc_quant_" + s for s in ("new", "free", "classes", "observed", "permute", "perm_rows", "gram_ms")}
    for name in declared:
        assert name in _lib.EXPORTS
    assert assocquant.MAX_COVAR == Q.MAX_COVAR == int(re.search(r"#define HIBAG_HIP_GLM_MAX_COVAR\s+(\d+)", hdr).group(1))
    assert assocquant.FLAG_RANK == Q.RANK_BIT == int(re.search(r"#define HIBAG_HIP_QUANT_RANK\s+(\d+)", hdr).group(1))
