"""hlaAssocHaplo on the host: the restatement of DESIGN.md section 30 (tests/assochaplo_reference.py) -- the posterior dosage
against sums written out here, the score test on real rows against numpy's least squares and solve and against the int8
restatement where the dosages are integers --, ``as_alleles``, the ``rare`` row, every argument error, hlaAssocHaplo end to
end on the restatement, and the safety conditions of the GPU comparisons.

Bound against lstsq / solve and against the int8 restatement: ten times the largest difference measured here, never looser
than 1e-9 (the measured values are in DESIGN.md section 30, "Checks", and printed by the tests)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assocglm_reference as G  # noqa: E402
import assochaplo_reference as HR  # noqa: E402
import assocscore_reference as SR  # noqa: E402
import haplo_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, assochaplo, haplo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA = R.NA
B = HR.Backend

BOUND_LSTSQ = 8.9e-14      # measured 8.91e-15 (single rows and sets, observed and under explicit signs, against lstsq / solve; in max(|T|, 1))
BOUND_INT8 = BOUND_LSTSQ   # measured 0 (integer dosages: the real-row restatement against the int8 one, relative; the same bound)


def hand_cohort():
    h1 = np.array([[[0, 0], [0, NA], [0, 1]], [[2, 2], [2, NA], [3, NA]]], np.int32)
    h2 = np.array([[[1, 0], [0, NA], [1, 1]], [[3, 2], [2, NA], [3, NA]]], np.int32)
    prob = np.array([[[.7, .3], [1., 0.], [.9, .1]], [[.6, .4], [1., 0.], [1., 0.]]])
    return h1, h2, prob


# 1 the dosage ----------------------------------------------------------------------------------------------------------------
def test_dosage_of_three_samples_by_hand():
    r = HR.dosages(*hand_cohort())
    # sample 0: states 0 .. 4 = (01, 23) in two phases, (01, 22), (00, 23), (00, 22); sample 1: state 5; sample 2: states 6, 7
    assert r["first"] == [0, 5, 6, 8] and r["keys"].tolist() == [2048, 2049, 3072, 3073]
    q = [float(v) for v in r["q"]]
    assert q[5] == 1.0
    # the lists in entry order (tests/test_hip_haplo.py): (0,2): s0 A, s2 A, s3 A, s4 A, s4 B, sample 1's state twice; (1,2): s1 B,
    # s2 B; (0,3): s1 A, s3 B, s6 A; (1,3): s0 B, s6 B, s7 A, s7 B
    assert r["lists"] == [[0, 4, 6, 8, 9, 10, 11], [3, 5], [2, 7, 12], [1, 13, 14, 15]]
    want = np.zeros((4, 3))
    want[0, 0] = ((((0.0 + q[0]) + q[2]) + q[3]) + q[4]) + q[4]
    want[0, 1] = (0.0 + q[5]) + q[5]
    want[1, 0] = (0.0 + q[1]) + q[2]
    want[2, 0] = (0.0 + q[1]) + q[3]
    want[2, 2] = 0.0 + q[6]
    want[3, 0] = 0.0 + q[0]
    want[3, 2] = ((0.0 + q[6]) + q[7]) + q[7]
    assert r["D"].tobytes() == want.tobytes()
    assert want[0, 1] == 2.0 and r["D"][1, 1] == 0.0 and r["D"][0, 2] == 0.0       # one state, homozygous: exactly 2; absent: exactly 0


def test_dosages_sum_to_two_and_one_state_samples_are_exact():
    _, h1, h2, prob = R.ld_cohort(130, 3, 3, 8, 12, seed=11)
    h1[1, 5, :] = NA; h2[1, 5, :] = NA; prob[1, 5, :] = 0.0                   # a sample left out
    for l in range(3):                                                        # an all-homozygous sample, a sample of one het state
        h1[l, 7, :], h2[l, 7, :], prob[l, 7, :] = [l + 1, NA, NA], [l + 1, NA, NA], [1.0, 0.0, 0.0]
        h1[l, 9, :], h2[l, 9, :], prob[l, 9, :] = [l + 1, NA, NA], [l + 1 + (l == 0), NA, NA], [1.0, 0.0, 0.0]
    r = HR.dosages(h1, h2, prob)
    D = r["D"]
    assert np.isnan(D[:, 5]).all() and not np.isnan(np.delete(D, 5, axis=1)).any()
    assert sorted(D[:, 7][D[:, 7] != 0].tolist()) == [2.0] and sorted(D[:, 9][D[:, 9] != 0].tolist()) == [1.0, 1.0]
    entries = 2 * r["n_states"]
    worst = 0.0
    for i in np.flatnonzero(r["used"]):
        gap = abs(float(D[:, i].sum()) - 2.0)
        worst = max(worst, gap / (entries[i] * np.spacing(2.0)))
        assert gap <= 4 * np.spacing(2.0) * entries[i], (i, gap, entries[i])
    print(f"sum of dosages: worst {worst:.3g} of an ulp of 2 per entry")
    assert (D[:, r["used"]] >= 0).all() and (D[:, r["used"]] <= 2.0 + 1e-12).all()


# 2 the real-row statistic, independently ---------------------------------------------------------------------------------------
def brute(Z, y, covar, sign_rows):
    """T [n_sets, P] from lstsq and solve: x~ = the residual of sqrt(w) x on sqrt(w) Z, U = x~'(e o s), V = x~' W x~, with mu
    from the converged base fit of tests/assocglm_reference.py."""
    n = len(y)
    Zm = np.column_stack([np.ones(n)] + list(covar))
    base = G.fit(Zm, y, np.ones(n))
    assert base["flags"] == 0
    mu = 1.0 / (1.0 + np.exp(-(Zm @ base["coef"])))
    w, e = mu * (1 - mu), y - mu
    sw = np.sqrt(w)
    out = np.full((len(Z.sets), len(sign_rows)), np.nan)
    for t, rows in enumerate(Z.kept_rows):
        if not rows:
            continue
        X = Z.F[rows].T
        Xt = (sw[:, None] * X - (sw[:, None] * Zm) @ np.linalg.lstsq(sw[:, None] * Zm, sw[:, None] * X, rcond=None)[0]) / sw[:, None]
        V = Xt.T @ (Xt * w[:, None])
        U = Xt.T @ (e[None, :] * sign_rows).T
        out[t] = (U * np.linalg.solve(V, U)).sum(axis=0)
    return out


@pytest.mark.parametrize("case", ["n40", "n257", "n1000"])
def test_real_rows_equal_lstsq_and_solve_under_every_sign_row(case):
    Z = HR.reference(case)
    A, covar, _, _ = SR.analysis(case, "additive")
    sg = SR.signs(Z.seed, 0, 1 + SR.N_PERM[case], A.n).astype(np.float64)
    want = brute(Z, A.y, covar, sg)
    got = np.concatenate([Z.stat[:, None], Z.perm_T], axis=1).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    gap = float(np.max(np.abs(got - want)[ok] / np.fmax(np.abs(want[ok]), 1)))
    print(f"{case}: real rows against lstsq / solve {gap:.3g}, sets of {sorted(set(Z.df.tolist()))} columns")
    assert gap <= BOUND_LSTSQ
    m = HR.ROWS[case]
    if m >= 4:                # the aliased set: row 0 kept; twice row 0, the constant and the zero row dropped
        t = Z.sets.index([0, m - 2, m - 3, m - 1])
        assert Z.kept[t] == 1 and Z.df[t] == 1 and Z.flags[t] == SR.ALIASED_BIT
        assert Z.flags[m - 1] == SR.RANK_BIT and Z.flags[m - 3] == SR.RANK_BIT and np.isnan(Z.stat[m - 1])
        assert Z.flags[Z.sets.index([])] == SR.RANK_BIT


# 3 integer dosages are the int8 path ---------------------------------------------------------------------------------------------
def one_state_cohort(n=90, seed=4):
    """k = 1 and at most one heterozygous locus: one state a sample, so that every dosage is 0.0, 1.0 or 2.0."""
    rng = np.random.default_rng(seed)
    L = 2
    a = rng.integers(0, 3, size=(L, n))
    b = a.copy()
    for s in range(n):
        l = int(rng.integers(0, L + 1))
        if l < L:
            b[l, s] = (a[l, s] + 1) % 3
    return np.minimum(a, b)[:, :, None].astype(np.int32), np.maximum(a, b)[:, :, None].astype(np.int32), np.ones((L, n, 1))


def test_integer_dosages_agree_with_the_int8_restatement():
    h1, h2, prob = one_state_cohort()
    res, r = HR.haplo_result(h1, h2, prob, 3, dosage_min_freq=0.0)
    D = r["D"]
    assert set(np.unique(D).tolist()) <= {0.0, 1.0, 2.0} and (D.sum(axis=0) == 2.0).all()
    rng = np.random.default_rng(8)
    n = D.shape[1]
    y = (rng.random(n) < 0.45).astype(np.int32)
    cov = rng.standard_normal((2, n))
    sets = [[j] for j in range(len(D))] + [list(range(len(D) - 1))]
    real = HR.RealScore(D, y, cov).install(sets)
    int8 = SR.Score(D.astype(np.int64), y, cov).install(sets)
    assert np.array_equal(real.df, int8.df) and np.array_equal(real.flags, int8.flags) and np.array_equal(real.kept, int8.kept)
    ok = ~np.isnan(int8.stat)
    gap = float(np.max(np.abs(real.stat[ok] / int8.stat[ok] - 1)))
    print(f"integer dosages: real rows against int8 rows {gap:.3g}")
    assert ok.sum() >= 3 and gap <= BOUND_INT8
    # and through the entries: expected == best on this cohort, test for test
    e = hb.hlaAssocHaplo(res, y, cov.T, min_freq=0.0, _backend=B)
    b = hb.hlaAssocHaplo(res, y, cov.T, min_freq=0.0, dosage="best", _backend=B)
    assert e.name == b.name and np.array_equal(e.df, b.df)
    fin = ~np.isnan(b.score_stat)
    assert np.max(np.abs(e.score_stat[fin] / b.score_stat[fin] - 1)) <= BOUND_INT8
    assert np.allclose(e.mean_dosage, b.mean_dosage, rtol=0, atol=1e-15) and np.array_equal(e.freq, b.freq)


# 4 as_alleles, rare, arguments ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    h1, h2, prob, n_allele, y, cov = HR.e2e_cohort()
    res, r = HR.haplo_result(h1, h2, prob, n_allele, dosage_min_freq=0.01)
    return res, r, y, cov


def test_as_alleles_and_the_rare_row(e2e):
    res, r, y, cov = e2e
    hla = res.as_alleles(0.05)
    sel = np.flatnonzero(res.freq >= 0.05)
    assert hla._levels == [res.names(int(i)) for i in sel] + ["rare"] and hla.locus == "L0~L1~L2"
    assert len(sel) >= 2 and len(sel) < len(res.freq)
    key_of = lambda h: [sum(int(a) << (10 * l) for l, a in enumerate(row)) for row in h]      # noqa: E731
    for h, got in ((res.h1, hla.h1), (res.h2, hla.h2)):
        want = [list(res.keys[sel]).index(k) if k in res.keys[sel] else len(sel) for k in key_of(h)]
        assert got.tolist() == want
    assert (hla.h1 == len(sel)).any() or (hla.h2 == len(sel)).any()                       # somebody carries a rare haplotype
    assert hla.allele1[0] in hla._levels and np.array_equal(hla.prob, res.prob, equal_nan=True)
    # a sample left out is NA
    h1, h2, prob = (a.copy() for a in hand_cohort())
    h1[1, 1, :] = NA; h2[1, 1, :] = NA; prob[1, 1, :] = 0.0
    small, _ = HR.haplo_result(h1, h2, prob, 4, dosage_min_freq=0.0)
    a = small.as_alleles(0.0)
    assert a.h1[1] == NA and a.h2[1] == NA and a.allele1[1] is None and np.isnan(small.dosage[:, 1]).all()
    assert a._levels[-1] == "rare" and len(a._levels) == len(small.freq) + 1
    with pytest.raises(ValueError, match="min_freq"):
        res.as_alleles(1.5)
    # rare = (2 - d_0) - d_1 - ... in order
    Dm = np.array([[0.25, 1.0], [0.5, 0.125], [1e-17, 0.5]])
    assert assochaplo.rare_row(Dm).tolist() == [((2.0 - 0.25) - 0.5) - 1e-17, ((2.0 - 1.0) - 0.125) - 0.5]


def test_hla_assoc_haplo_on_the_restatement(e2e):
    res, r, y, cov = e2e
    out = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, n_perm=40, seed=HR.E2E_SEED, _backend=B)
    sel = np.flatnonzero(res.freq >= 0.02)
    assert out.name == [res.names(int(i)) for i in sel] and np.array_equal(out.freq, res.freq[sel]) and out.dosage == "expected"
    used = res.used
    at = {int(i): k for k, i in enumerate(res.dosage_index)}
    D = np.ascontiguousarray(res.dosage[[at[int(i)] for i in sel]][:, used])
    assert np.allclose(out.mean_dosage, D.mean(axis=1), rtol=1e-14) and out.n_samp == used.sum()
    assert abs(out.mean_dosage[0] / 2 - res.freq[0]) < 0.02                                # the mean dosage is twice the frequency
    # the same numbers from the restatement driven directly
    Z = HR.RealScore(D, y[used], np.ascontiguousarray(cov[used].T)).install([[j] for j in range(len(D))])
    assert out.score_stat.tobytes() == Z.stat.astype(np.float64).tobytes() and np.array_equal(out.df, Z.df)
    assert (out.df == 1).all() and out.score_p.min() < 0.01                                # the planted effect is found
    assert out.name[int(np.nanargmax(out.score_stat))] == res.names(0)
    assert out.perm_p.shape == out.perm_p_adj.shape == (len(sel),) and (out.perm_p_adj >= out.perm_p - 1e-15).all()
    assert set(out.to_table()) == {"freq", "mean.dosage", "df", "score.st", "score.p", "perm.p", "perm.p.adj"}
    assert "HlaAssocHaploResult('expected'" in repr(out)
    # conditioned on the top hit: its own test is aliased away, its column is a covariate
    top = res.names(0)
    c = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, condition=[top], _backend=B)
    assert c.flags[0] & SR.RANK_BIT and np.isnan(c.score_stat[0]) and c.base["name"][-1] == f"h[{top}]"
    assert np.isfinite(c.score_stat[1:]).all()
    # omnibus: one set of the selected haplotypes without the first, plus rare
    o = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, omnibus=True, _backend=B)
    rows = np.concatenate([D[1:], assochaplo.rare_row(D)[None, :]])
    Zo = HR.RealScore(rows, y[used], np.ascontiguousarray(cov[used].T)).install([list(range(len(rows)))])
    assert o.name == ["omnibus"] and o.df[0] == Zo.df[0] == len(rows) and o.score_stat[0] == float(Zo.stat[0])
    ob = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, omnibus=True, dosage="best", _backend=B)
    assert ob.df[0] >= 1 and np.isfinite(ob.score_stat[0])
    # best: hlaAssocScore on as_alleles, bit for bit
    b = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, dosage="best", n_perm=40, seed=HR.E2E_SEED, _backend=B)
    s = hb.hlaAssocScore(res.as_alleles(0.02), y, cov, model="additive", n_perm=40, seed=HR.E2E_SEED, _backend=B)
    pick = [s.name.index(n) for n in b.name]
    for key in ("score_stat", "score_p", "perm_p", "perm_p_adj", "df", "flags"):
        assert np.asarray(getattr(b, key)).tobytes() == np.asarray(getattr(s, key))[pick].tobytes(), key
    assert b.max_stat.tobytes() == s.max_stat.tobytes()


def test_argument_errors(e2e):
    res, r, y, cov = e2e
    plain, _ = HR.haplo_result(*hand_cohort(), 4)
    assert plain.dosage is None and plain.dosage_index is None and plain.dosage_min_freq is None
    with pytest.raises(ValueError, match="dosage_min_freq"):
        hb.hlaAssocHaplo(plain, [0, 1, 1], min_freq=0.0, _backend=B)
    with pytest.raises(ValueError, match="below the result's dosage_min_freq"):
        hb.hlaAssocHaplo(res, y, cov, min_freq=0.005, _backend=B)
    with pytest.raises(ValueError, match="dosage must be"):
        hb.hlaAssocHaplo(res, y, cov, dosage="posterior", _backend=B)
    with pytest.raises(TypeError):
        hb.hlaAssocHaplo(res.as_alleles(0.02), y, cov, _backend=B)
    with pytest.raises(ValueError, match="min_freq"):
        hb.hlaAssocHaplo(res, y, cov, min_freq=-1, _backend=B)
    with pytest.raises(ValueError, match="no haplotype"):
        hb.hlaAssocHaplo(res, y, cov, min_freq=0.999, _backend=B)
    with pytest.raises(ValueError, match="not a haplotype"):
        hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, condition=["L0*0000~nothing"], _backend=B)
    with pytest.raises(ValueError, match="covariate columns"):
        hb.hlaAssocHaplo(res, y, np.random.default_rng(0).standard_normal((200, 12)), min_freq=0.02, condition=[res.names(0)], _backend=B)
    with pytest.raises(ValueError):
        hb.hlaAssocHaplo(res, y[:-1], cov, min_freq=0.02, _backend=B)
    with pytest.raises(ValueError):
        hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, n_perm=-1, _backend=B)
    # more than 30 columns in the omnibus set
    _, h1, h2, prob = R.ld_cohort(400, 2, 1, 40, 30, seed=3)
    wide, _ = HR.haplo_result(h1, h2, prob, 30, dosage_min_freq=0.0)
    assert len(wide.freq) > 30
    with pytest.raises(ValueError, match="at most 30"):
        hb.hlaAssocHaplo(wide, np.arange(400) % 2, min_freq=0.0, omnibus=True, _backend=B)
    with pytest.raises(ValueError, match="dosage_min_freq"):
        hb.hlaHaplotypes({}, dosage_min_freq=2.0)


# 5 the safety conditions of the GPU comparisons -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(HR.ROWS))
def test_no_resampled_statistic_near_the_observed_one(case):
    """Every |T[t][p] - T[t][0]| of every case tests/test_hip_assochaplo.py compares exceeds 1e-6 T[t][0], every |min_p[p] -
    score_p[t]| exceeds 1e-6 score_p[t], no pivot ratio lies between 1e-13 and 1e-9, and the seed is the first that does."""
    Z = HR.reference(case)
    assert Z.perm_T.shape[1] == SR.N_PERM[case]
    g_stat, g_p = SR.min_gap(Z, Z.perm_T)
    print(f"{case}: closest statistic gap {g_stat:.3g}, closest p-value gap {g_p:.3g}, tolerance {HR.tolerance(case):.3g}")
    assert g_stat > SR.SAFETY and g_p > SR.SAFETY and np.isfinite(g_stat)
    assert all(r < 1e-13 or r > 1e-9 for r in Z.ratios)
    for k in range(HR.SEEDS.get(case, 0)):
        earlier = HR.reference(case, seed=SR.PERM_SEED + k)
        assert min(SR.min_gap(earlier, earlier.perm_T)) <= SR.SAFETY
    sizes = {len(s) for s in Z.sets}
    assert {0, 1} <= sizes and (HR.ROWS[case] < 30 or {2, 15, 16, 17, 30} <= sizes)


def test_end_to_end_runs_meet_the_safety_condition(e2e):
    res, r, y, cov = e2e
    plain = hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, n_perm=200, seed=HR.E2E_SEED, _backend=B)
    runs = [plain, hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, condition=[res.names(0)], n_perm=200, seed=HR.E2E_SEED, _backend=B),
            hb.hlaAssocHaplo(res, y, cov, min_freq=0.02, omnibus=True, n_perm=200, seed=HR.E2E_SEED, _backend=B)]
    for run in runs:
        with np.errstate(invalid="ignore", divide="ignore"):
            gp = np.abs(run.min_p[None, :] - run.score_p[:, None]) / run.score_p[:, None]
        assert np.nanmin(gp) > SR.SAFETY and np.isfinite(run.perm_p_adj).sum() >= 1


# 6 the interface ------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    for name in ("hibag_hip_haplo_dosage", "hibag_hip_assoc_rscore_sets"):
        assert name in _lib.EXPORTS and re.search(r"\b" + name + r"\(", header), name
        assert hasattr(_lib.lib(), name)
    for name in ("hlaAssocHaplo", "HlaAssocHaploResult"):
        assert name in hb.__all__ and getattr(hb, name) is getattr(assochaplo, name)
    assert "association tests on haplotypes" not in haplo.__doc__.split("Not built")[1].split("(")[0]
