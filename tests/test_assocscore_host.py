"""hlaAssocScore on the host: the restatement of DESIGN.md section 28 (tests/assocscore_reference.py) against the closed forms
of the score test (Pearson's chi-square, the Cochran-Armitage trend test), against numpy's least squares and solve on the
full design, and against the same brute force under explicit signs; the invariance of the omnibus statistic; the sign
generator; the replicates' first moment; the NaN, aliased and RANK rules; hlaAssocScore's own host side (condition, the
non-converged base fit, every ValueError) end to end on the restatement; and the safety condition of the GPU comparisons.

Bounds against the closed forms, lstsq and solve: ten times the largest difference measured here, never looser than 1e-9
relative (the measured values are in DESIGN.md section 28, "Checks", and printed by the tests)."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assocglm_reference as G  # noqa: E402
import assocscore_reference as SR  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assoc, assocscore  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = SR.Backend

# measured on the cases below -> the bound (10 x measured, at most 1e-9)
BOUND_PEARSON = 1.9e-13     # measured 1.87e-14 (dominant score_stat against N (ad - bc)^2 / (r1 r2 c1 c2), relative; base fit run to epsilon 1e-14)
BOUND_TREND = 3.3e-13       # measured 3.3e-14 (additive score_stat against the Cochran-Armitage statistic in its N form, relative)
BOUND_LSTSQ = 2.2e-13       # measured 2.19e-14 (single tests and sets against lstsq / solve at the same base fit, relative)
BOUND_SIGNS = 1.3e-13       # measured 1.23e-14 (every T[t][p] against the same brute force under explicit signs, in max(|T|, 1))
BOUND_REFERENCE = 2.2e-13   # measured 2.2e-14 (the omnibus statistic with each carried level left out in turn, relative)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.fmax(np.abs(b[ok]), 1e-300), initial=0.0))


# 1 closed forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n40", "n1000"])
def test_dominant_without_covariates_is_pearsons_chi_square(case):
    hla, y, groups, _ = SR.hla_of(case)
    res = hb.hlaAssocScore(hla, y, None, "dominant", groups=groups, epsilon=1e-14, _backend=B)      # (the base fit run to the end)
    A = SR.analysis(case, "dominant")[0]
    a, b, c, d = (A.tab[:, k].astype(np.float64) for k in range(4))                # without / with x control / case
    with np.errstate(divide="ignore", invalid="ignore"):
        want = (a + b + c + d) * (a * d - b * c) ** 2 / ((a + b) * (c + d) * (a + c) * (b + d))
    want[(A.rsum == 0) | (A.rsum == A.n)] = np.nan
    got = res.score_stat[:len(want)]
    gap = rel(got, want)
    print(f"{case}: Pearson gap {gap:.3g}")
    assert gap <= BOUND_PEARSON and np.isfinite(want).sum() >= 5
    assert (res.df[:len(want)] == np.isfinite(want)).all()


@pytest.mark.parametrize("case", ["n40", "n1000"])
def test_additive_without_covariates_is_the_trend_test(case):
    hla, y, groups, _ = SR.hla_of(case)
    res = hb.hlaAssocScore(hla, y, None, "additive", groups=groups, epsilon=1e-14, _backend=B)
    A = SR.analysis(case, "additive")[0]
    x, yy, N = A.F.astype(np.float64), A.y.astype(np.float64), float(A.n)
    sx, sy = x.sum(axis=1), yy.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = N * (N * (x @ yy) - sx * sy) ** 2 / (sy * (N - sy) * (N * (x * x).sum(axis=1) - sx * sx))
    want[(A.rsum == 0) | (A.rsum == 2 * A.n)] = np.nan
    gap = rel(res.score_stat[:len(want)], want)
    print(f"{case}: Cochran-Armitage gap {gap:.3g}")
    assert gap <= BOUND_TREND and np.isfinite(want).sum() >= 5


# 2 the statistic, independently ---------------------------------------------------------------------------------------------
def brute(Z, A, covar, sign_rows):
    """T [n_sets, P] from lstsq and solve: x~ = the residual of sqrt(w) x on sqrt(w) Z, U = x~'(e o s), V = x~' W x~, with mu
    from the converged base fit of tests/assocglm_reference.py."""
    n = A.n
    Zm = np.column_stack([np.ones(n)] + list(covar))
    base = G.fit(Zm, A.y, np.ones(n))
    assert base["flags"] == 0
    mu = 1.0 / (1.0 + np.exp(-(Zm @ base["coef"])))
    w, e = mu * (1 - mu), A.y - mu
    sw = np.sqrt(w)
    out = np.full((len(Z.sets), len(sign_rows)), np.nan)
    for t, rows in enumerate(Z.kept_rows):
        if not rows:
            continue
        X = A.F[rows].astype(np.float64).T
        Xt = (sw[:, None] * X - (sw[:, None] * Zm) @ np.linalg.lstsq(sw[:, None] * Zm, sw[:, None] * X, rcond=None)[0]) / sw[:, None]
        V = Xt.T @ (Xt * w[:, None])
        U = Xt.T @ (e[None, :] * sign_rows).T                        # [d, P]
        out[t] = (U * np.linalg.solve(V, U)).sum(axis=0)
    return out


@pytest.mark.parametrize("case,model", [("n255", "dominant"), ("n257", "genotype"), ("n1000", "additive"), ("n1000", "recessive")])
def test_statistics_equal_lstsq_and_solve_under_every_sign_row(case, model):
    Z = SR.reference(case, model)
    A, covar, _, _ = SR.analysis(case, model)
    sg = SR.signs(Z.seed, 0, 1 + SR.N_PERM[case], A.n).astype(np.float64)
    assert (sg[0] == 1).all()
    want = brute(Z, A, covar, sg)
    got = np.concatenate([Z.stat[:, None], Z.perm_T], axis=1).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    gap_obs = float(np.max(np.abs(got[:, 0] - want[:, 0])[ok[:, 0]] / np.abs(want[:, 0])[ok[:, 0]]))
    gap_all = float(np.max(np.abs(got - want)[ok] / np.fmax(np.abs(want[ok]), 1)))
    print(f"{case} {model}: observed gap {gap_obs:.3g}, all replicates {gap_all:.3g}, sets of {sorted(set(Z.df.tolist()))} columns")
    assert gap_obs <= BOUND_LSTSQ and gap_all <= BOUND_SIGNS


def test_the_omnibus_statistic_does_not_depend_on_the_reference_level():
    A, covar, _, _ = SR.analysis("n1000", "additive")
    n_allele = SR.CASES["n1000"][1]
    levels = [n_allele + lv for lv in (0, 2, 3)]                    # the carried levels of the gap partition
    Z = SR.Score(A.F, A.y, covar).install([[r for r in levels if r != out] for out in levels] + [list(range(1, 9)), [0] + list(range(2, 9))])
    sg = SR.signs(5, 0, 40, A.n)
    T = Z.run(sg)[1].astype(np.float64)
    assert (Z.df[:3] == 2).all() and np.isfinite(T).all()
    gap = max(np.max(np.abs(T[k] / T[0] - 1)) for k in (1, 2))
    print(f"reference level: gap {gap:.3g}")
    assert gap <= BOUND_REFERENCE
    # (eight alleles of 65 do not sum to a constant: leaving another one out is another test)
    assert np.max(np.abs(T[4] / T[3] - 1)) > 1e-3


# 3 the generator --------------------------------------------------------------------------------------------------------------
def test_generator():
    seed = 0x0123456789ABCDEF
    # by hand: sample 3 under key (0x89ABCDEF, 0x01234567): Philox4x32-10(counter (3, 2, 0, 0)) = febf243f a6892562 0c1c4f91
    # a3856d72 and (3, 2, 1, 0) = 8466087c ...; replicate 1 is bit 1 of word 0 of block 0 (set: -1), 127 bit 31 of word 3 (set),
    # 128 and 129 bits 0 and 1 of word 0 of block 1 (0x7c = 0111 1100: clear, clear)
    from draws_reference import philox4x32_10
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    assert [int(v) for v in philox4x32_10(np.array([[3, 2, 0, 0]], np.uint64), key)[0]] == [0xFEBF243F, 0xA6892562, 0x0C1C4F91, 0xA3856D72]
    assert int(philox4x32_10(np.array([[3, 2, 1, 0]], np.uint64), key)[0][0]) == 0x8466087C
    assert SR.signs(seed, 1, 1, 5)[0].tolist() == [1, -1, -1, -1, -1]
    assert SR.signs(seed, 127, 3, 5).tolist() == [[-1, -1, -1, -1, -1], [1, 1, -1, 1, 1], [-1, -1, -1, 1, 1]]
    assert SR.signs(seed, (1 << 39) + 5, 1, 5)[0].tolist() == [1, 1, -1, -1, -1]
    assert (SR.signs(seed, 0, 1, 5) == 1).all()                                    # replicate 0: the observed run
    big = SR.signs(seed, (1 << 39) + 120, 20, 50)                                  # a block boundary above 2^32 blocks' worth of p
    assert big.tobytes() == np.concatenate([SR.signs(seed, (1 << 39) + 120 + k, 1, 50) for k in range(20)]).tobytes()
    assert SR.signs(seed, (1 << 63) + 3, 2, 50).tobytes() != SR.signs(seed, 3, 2, 50).tobytes()       # (the block's high word counts)
    # ranges concatenate; a sign is a function of (seed, p, i) alone
    whole = SR.signs(77, 1, 200, 33)
    assert whole.tobytes() == np.concatenate([SR.signs(77, 1, 100, 33), SR.signs(77, 101, 100, 33)]).tobytes()
    assert SR.signs(77, 1, 200, 40)[:, :33].tobytes() == whole.tobytes()
    assert SR.signs(78, 1, 200, 33).tobytes() != whole.tobytes()
    # frequencies: every sample's and every replicate's mean sign within 5 standard errors of 0
    s = SR.signs(2024, 1, 4000, 300).astype(np.float64)
    assert set(np.unique(s)) == {-1.0, 1.0}
    assert np.abs(s.mean(axis=0)).max() <= 5 / math.sqrt(4000) and np.abs(s.mean(axis=1)).max() <= 5 / math.sqrt(300)
    assert abs(s.mean()) <= 5 / math.sqrt(s.size)
    c = np.corrcoef(s[:, :40].T)
    assert np.abs(c - np.eye(40)).max() <= 5 / math.sqrt(4000)


# 4 moments --------------------------------------------------------------------------------------------------------------------
def test_the_replicates_mean_is_the_sandwich_ratio():
    """E T* = sum e_i^2 x~_i^2 / V for a one-column test: over 4,000 replicates every test's mean lies within 5 standard
    errors of it."""
    A, covar, _, _ = SR.analysis("n257", "dominant")
    Z = SR.Score(A.F, A.y, covar).install(SR.single_sets("dominant", A.rsum, A.n))
    T = Z.stats(99, 1, 4000).astype(np.float64)
    checked = 0
    for t, rows in enumerate(Z.kept_rows):
        if not rows:
            continue
        x = A.F[rows[0]].astype(np.float64)
        xt = x - Z.Q.T.astype(np.float64) @ Z.proj[rows[0]].astype(np.float64)
        V = float((Z.w * xt * xt).sum())
        want = float((Z.e * Z.e * xt * xt).sum()) / V
        se = T[t].std(ddof=1) / math.sqrt(T.shape[1])
        assert abs(T[t].mean() - want) <= 5 * se, (t, T[t].mean(), want, se)
        assert abs(float(Z.L[t][0][0]) ** 2 / V - 1) <= 1e-9
        checked += 1
    assert checked >= 10


# 5 rules ----------------------------------------------------------------------------------------------------------------------
def test_nan_aliased_and_rank_rules():
    A, covar, _, _ = SR.analysis("n1000", "additive")
    n_allele = SR.CASES["n1000"][1]
    gap = [n_allele + lv for lv in range(4)]
    assert A.rsum[gap[1]] == 0
    cov = np.concatenate([covar, A.F[3:4].astype(np.float64)])                      # conditioned on allele 3
    sets = [[0], [], [gap[1]], [gap[0], gap[1], gap[2]], [3], [3, 4], [4, 3], list(range(n_allele))[:30], [gap[0], gap[2], gap[3]]]
    Z = SR.Score(A.F, A.y, cov).install(sets)
    assert Z.flags.tolist() == [0, 2, 2, 8, 2, 8, 8, 8, 8] and Z.df.tolist() == [1, 0, 0, 2, 0, 1, 1, 29, 2]
    assert Z.kept.tolist() == [1, 0, 0, 0b101, 0, 0b10, 0b01, (1 << 30) - 1 - (1 << 3), 0b011]
    assert np.isnan(Z.stat[[1, 2, 4]]).all() and np.isfinite(Z.stat[[0, 3, 5, 6, 7, 8]]).all()
    assert abs(Z.stat[5] / Z.stat[6] - 1) <= 1e-9                                   # the aliased column adds nothing, wherever it stands
    assert all(r < 1e-13 or r > 1e-9 for r in Z.ratios)                             # (no pivot near the threshold 1e-11)
    T = Z.stats(3, 1, 20)
    assert np.isnan(T[[1, 2, 4]]).all() and np.isfinite(np.delete(T, [1, 2, 4], axis=0)).all()
    max_stat, count = Z.max_and_count(T)
    assert Z.dfs == [1, 2, 29] and max_stat.shape == (20, 3) and (count[[1, 2, 4]] == 0).all()
    assert np.array_equal(max_stat[:, 0], np.fmax(np.fmax(T[0], T[5]), T[6])) and np.array_equal(max_stat[:, 2], T[7])
    # every kind of column through the entry: a constant column and a level nobody carries are RANK and NaN
    hla, y, groups, covm = SR.hla_of("n1000")
    for model in SR.MODELS:
        res = hb.hlaAssocScore(hla, y, covm, model, groups=groups, n_perm=16, seed=4, _backend=B)
        An = SR.analysis("n1000", model)[0]
        want_sets = SR.single_sets(model, An.rsum, An.n)
        dead = np.array([not s for s in want_sets] + [True])                       # ... and "pos:beyond", unknown to the device
        assert res.name[-1] == "pos:beyond" and len(res.name) == len(dead)
        assert ((res.flags & 2) != 0).tolist() == dead.tolist() and np.isnan(res.score_stat[dead]).all()
        assert np.isnan(res.score_p[dead]).all() and np.isnan(res.perm_p[dead]).all() and np.isnan(res.perm_p_adj[dead]).all()
        assert np.isfinite(res.score_stat[~dead]).all() and (res.df[dead] == 0).all()
        assert res.df[~dead].tolist() == [len(s) for s in want_sets if s]
        assert ((res.perm_p[~dead] >= 1 / 17) & (res.perm_p[~dead] <= 1)).all() and (res.perm_p_adj[~dead] >= res.perm_p[~dead]).all()
        assert res.max_stat.shape == (16, len(res.max_stat_df)) and res.min_p.shape == (16,) and res.seed == 4 and res.n_perm == 16


def test_p_values_from_counts():
    hla, y, groups, covm = SR.hla_of("n255")
    res = hb.hlaAssocScore(hla, y, covm, "genotype", n_perm=60, seed=8, _backend=B)
    A, covar, _, _ = SR.analysis("n255", "genotype")
    Z = SR.Score(A.F, A.y, covar).install(SR.single_sets("genotype", A.rsum, A.n))
    T = Z.stats(8, 1, 60).astype(np.float64)
    assert {1, 2} <= set(Z.df.tolist()) <= {0, 1, 2} and res.max_stat_df.tolist() == [1, 2]
    p = np.array([[assoc.chisq_sf(float(v), int(d)) if d else np.nan for v in row] for row, d in zip(T, Z.df)])
    min_p = np.nanmin(p, axis=0)
    assert np.array_equal(res.min_p, min_p)
    ok = Z.df > 0
    sp = np.array([assoc.chisq_sf(float(v), int(d)) if d else np.nan for v, d in zip(Z.stat, Z.df)])
    assert np.array_equal(res.score_p, sp, equal_nan=True)
    assert np.array_equal(res.perm_p[ok], (1 + (T[ok] >= Z.stat[ok, None].astype(np.float64)).sum(axis=1)) / 61)
    assert np.array_equal(res.perm_p_adj[ok], (1 + (min_p[None, :] <= sp[ok, None]).sum(axis=1)) / 61)
    assert set(res.to_table()) == {"df", "score.st", "score.p", "perm.p", "perm.p.adj"} and "60 replicates" in repr(res)
    assert set(hb.hlaAssocScore(hla, y, covm, _backend=B).to_table()) == {"df", "score.st", "score.p"}


def test_chisq_sf_array_equals_the_scalar_function():
    x = np.concatenate([[np.nan, 0.0, -1.0, 1e-300, 745.0, 1500.0], np.random.default_rng(1).gamma(2.0, 6.0, 300)])
    for df in list(range(1, 32)) + [0]:
        want = np.array([assoc.chisq_sf(float(v), df) for v in x])
        assert np.array_equal(assocscore.chisq_sf_array(x, df), want, equal_nan=True), df
    assert assocscore.chisq_sf_array(np.zeros((2, 0)), 3).shape == (2, 0)


# 6 the entry ------------------------------------------------------------------------------------------------------------------
def test_condition_and_omnibus():
    hla, y, groups, covm = SR.hla_of("n1000")
    plain = hb.hlaAssocScore(hla, y, covm, groups=groups, _backend=B)
    top = plain.name[int(np.nanargmax(plain.score_stat))]
    cond = hb.hlaAssocScore(hla, y, covm, groups=groups, condition=top, _backend=B)
    assert cond.base["name"] == ["(Intercept)"] + [f"c{k + 1}" for k in range(6)] + [f"h[{top}]"]
    k = plain.name.index(top)
    assert cond.flags[k] == 2 and math.isnan(cond.score_stat[k]) and cond.df[k] == 0      # the conditioned test itself is aliased
    assert np.isfinite(cond.base["est"]).all() and cond.base["flags"] == 0
    gen = hb.hlaAssocScore(hla, y, covm, "genotype", condition=[top], _backend=B)
    assert gen.base["name"][-2:] == [f"h1[{top}]", f"h2[{top}]"] and gen.flags[k] == 2
    om = hb.hlaAssocScore(hla, y, covm, "additive", groups=groups, omnibus=True, n_perm=20, seed=1, _backend=B)
    assert om.name == ["pos"] and om.df.tolist() == [2] and om.n_levels.tolist() == [3] and om.reference == ["x"] and om.omnibus
    assert "1 partitions" in repr(om)
    # a set with an aliased level: conditioned on one of its own levels; conditioned on the whole partition
    one = hb.hlaAssocScore(hla, y, covm, "additive", groups=groups, omnibus=True, condition=["pos:y"], _backend=B)
    assert one.df.tolist() == [1] and one.flags.tolist() == [8] and one.base["name"][-1] == "h[pos:y]"
    whole = hb.hlaAssocScore(hla, y, covm, "additive", groups=groups, omnibus=True, condition=["pos"], _backend=B)
    assert whole.df.tolist() == [0] and whole.flags.tolist() == [2] and whole.base["name"][-2:] == ["h[pos:y]", "h[pos:z]"]
    # the omnibus statistic of a two-level split is the single test's
    two = hb.HlaAlleleGroups(groups.alleles, ["half"], [["a", "b"]], (np.arange(len(groups.alleles)) % 2)[None, :].astype(np.int32))
    o2 = hb.hlaAssocScore(hla, y, covm, "additive", groups=two, omnibus=True, _backend=B)
    s2 = hb.hlaAssocScore(hla, y, covm, "additive", groups=two, _backend=B)
    assert abs(o2.score_stat[0] / s2.score_stat[s2.name.index("half:a")] - 1) <= 1e-9
    assert abs(o2.score_stat[0] / s2.score_stat[s2.name.index("half:b")] - 1) <= 1e-9


def test_a_base_fit_that_did_not_converge():
    hla, y, groups, covm = SR.hla_of("n257")
    res = hb.hlaAssocScore(hla, y, covm, n_perm=10, seed=2, maxit=1, _backend=B)
    assert res.base["flags"] & 1 and (res.flags & 1).all() and np.isnan(res.score_stat).all() and np.isnan(res.score_p).all()
    assert (res.df == 0).all() and np.isnan(res.perm_p).all() and np.isnan(res.perm_p_adj).all()
    assert res.max_stat.shape == (10, 0) and np.isnan(res.min_p).all()
    prob = hb.hlaAssocScore(hla, y, covm, use_prob=True, _backend=B)                 # prior weights without replicates
    assert prob.base["flags"] == 0 and np.isfinite(prob.score_stat).sum() >= 10
    assert not np.array_equal(prob.score_stat, hb.hlaAssocScore(hla, y, covm, _backend=B).score_stat, equal_nan=True)


def test_value_errors():
    hla, y, groups, covm = SR.hla_of("n1000")
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaAssocScore(hla, y, covm, "overdominant", _backend=B)
    with pytest.raises(ValueError, match="genotype coding"):
        hb.hlaAssocScore(hla, y, covm, "genotype", groups=groups, omnibus=True, _backend=B)
    with pytest.raises(ValueError, match="needs 'groups'"):
        hb.hlaAssocScore(hla, y, covm, omnibus=True, _backend=B)
    with pytest.raises(TypeError, match="HlaAlleleGroups"):
        hb.hlaAssocScore(hla, y, covm, groups=[1, 2], _backend=B)
    with pytest.raises(ValueError, match="section 28"):
        hb.hlaAssocScore(hla, y, covm, use_prob=True, n_perm=10, _backend=B)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="n_perm"):
            hb.hlaAssocScore(hla, y, covm, n_perm=bad, _backend=B)
    for bad in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            hb.hlaAssocScore(hla, y, covm, n_perm=4, seed=bad, _backend=B)
    with pytest.raises(ValueError, match="maxit"):
        hb.hlaAssocScore(hla, y, covm, maxit=0, _backend=B)
    with pytest.raises(ValueError, match="epsilon"):
        hb.hlaAssocScore(hla, y, covm, epsilon=0.0, _backend=B)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocScore(hla, y[:-1], covm, _backend=B)
    with pytest.raises(ValueError, match="covariate 'c1' has"):
        hb.hlaAssocScore(hla, y, covm[:-1], _backend=B)
    nanc = covm.copy()
    nanc[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        hb.hlaAssocScore(hla, y, nanc, _backend=B)
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocScore(hla, y, np.column_stack([covm[:, 0], 1 - 3 * covm[:, 0]]), _backend=B)
    with pytest.raises(ValueError, match="not a test of this analysis"):
        hb.hlaAssocScore(hla, y, covm, condition=["99:99"], _backend=B)
    with pytest.raises(ValueError, match="neither a partition nor a test"):
        hb.hlaAssocScore(hla, y, covm, "additive", groups=groups, omnibus=True, condition=["nowhere"], _backend=B)
    with pytest.raises(ValueError, match="no allele of the data"):
        hb.hlaAssocScore(hla, y, covm, groups=groups, condition=["pos:beyond"], _backend=B)
    with pytest.raises(ValueError, match="list of test names"):
        hb.hlaAssocScore(hla, y, covm, condition=[3], _backend=B)
    names = SR.allele_names(SR.CASES["n1000"][1])
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocScore(hla, y, covm, condition=names[:7], _backend=B)
    with pytest.raises(ValueError, match="at most 12"):
        hb.hlaAssocScore(hla, y, np.random.default_rng(0).standard_normal((len(y), 13)), _backend=B)
    every = hb.HlaAlleleGroups(groups.alleles, ["all"], [list(groups.alleles)], np.arange(len(groups.alleles))[None, :].astype(np.int32))
    with pytest.raises(ValueError, match="more than 30 columns"):
        hb.hlaAssocScore(hla, y, covm, "additive", groups=every, omnibus=True, _backend=B)
    with pytest.raises(ValueError, match="posterior probability"):
        hb.hlaAssocScore(hb.hlaAllele(hla.sample_id, hla.allele1, hla.allele2, locus="A"), y, covm, use_prob=True, _backend=B)
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaAssocScore("hla", y, covm, _backend=B)
    drawn = hb.hlaAssocScore(hla, y, covm, n_perm=3, _backend=B)
    assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 1 << 64 and hb.hlaAssocScore(hla, y, covm, _backend=B).seed is None


# 7 the safety condition of the GPU comparisons ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SR.MODELS)
@pytest.mark.parametrize("case", list(SR.CASES))
def test_no_resampled_statistic_near_the_observed_one(case, model):
    """Every |T[t][p] - T[t][0]| of every case tests/test_hip_assocscore.py compares exceeds 1e-6 T[t][0] and every
    |min_p[p] - score_p[t]| exceeds 1e-6 score_p[t], so that the device's `>=` and the restatement's agree whatever the last
    bits; no pivot lies near the drop threshold; and the seed is the first that does."""
    Z = SR.reference(case, model)
    assert Z.perm_T.shape[1] == SR.N_PERM[case] == max(SR.PERM_COUNTS[case])
    g_stat, g_p = SR.min_gap(Z, Z.perm_T)
    print(f"{case} {model}: closest statistic gap {g_stat:.3g}, closest p-value gap {g_p:.3g}, tolerance {SR.tolerance(case, model):.3g}")
    assert g_stat > SR.SAFETY and g_p > SR.SAFETY and np.isfinite(g_stat)
    assert all(r < 1e-13 or r > 1e-9 for r in Z.ratios)
    for k in range(SR.SEEDS.get((case, model), 0)):
        earlier = SR.reference(case, model, seed=SR.PERM_SEED + k)
        assert min(SR.min_gap(earlier, earlier.perm_T)) <= SR.SAFETY


def test_device_run_sets_cover_the_set_sizes():
    sizes, flags = set(), set()
    for case in SR.CASES:
        for model in SR.MODELS:
            Z = SR.reference(case, model)
            sizes |= {len(s) for s in Z.sets}
            flags |= set(Z.flags.tolist())
    assert {0, 1, 2, 15, 16, 17, 30} <= sizes and max(sizes) == 30 and {0, 2, 8} <= flags


def test_end_to_end_runs_meet_the_safety_condition():
    """The hlaAssocScore runs the GPU test compares: n1000 dominant, 65 replicates, plain, conditioned on the top hit, and
    the omnibus form."""
    hla, y, groups, covm = SR.hla_of("n1000")
    seed = SR.seed_of("n1000", "dominant")
    plain = hb.hlaAssocScore(hla, y, covm, groups=groups, n_perm=65, seed=seed, _backend=B)
    top = plain.name[int(np.nanargmax(plain.score_stat))]
    runs = [plain, hb.hlaAssocScore(hla, y, covm, groups=groups, condition=[top], n_perm=65, seed=seed, _backend=B),
            hb.hlaAssocScore(hla, y, covm, "additive", groups=groups, omnibus=True, n_perm=65, seed=seed, _backend=B)]
    for res in runs:
        with np.errstate(invalid="ignore", divide="ignore"):
            gp = np.abs(res.min_p[None, :] - res.score_p[:, None]) / res.score_p[:, None]
        assert np.nanmin(gp) > SR.SAFETY
        # perm_p = (1 + count) / 66 moves by 1 / 66 per tie: the counts of the restatement in longdouble are the same
        assert np.isfinite(res.perm_p_adj).sum() >= 1


# 8 the interface ----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    from hibag_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    declared = set(re.findall(r"\b(hibag_hip_assoc_score_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"hibag_hip_assoc_score_" + s for s in ("new", "free", "base", "sets", "observed", "n_df", "resample", "signs", "ms")}
    for name in declared:
        assert name in _lib.EXPORTS
    assert "hlaAssocScore" in hb.__all__ and "HlaAssocScoreResult" in hb.__all__ and hb.hlaAssocScore is assocscore.hlaAssocScore
    assert assocscore.MAX_ROWS == SR.MAX_ROWS == int(re.search(r"#define HIBAG_HIP_SCORE_MAX_ROWS\s+(\d+)", hdr).group(1))
    assert assocscore.MAX_COVAR == SR.MAX_COVAR == int(re.search(r"#define HIBAG_HIP_GLM_MAX_COVAR\s+(\d+)", hdr).group(1))
    assert (SR.MAXIT_BIT, SR.RANK_BIT, SR.ALIASED_BIT) == (assocscore.FLAG_MAXIT, assocscore.FLAG_RANK, 8)
    src = open(os.path.join(ROOT, "hibag_amd", "csrc", "Makefile")).read()
    assert "hibag_k_score.h" in src
