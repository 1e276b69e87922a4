"""hlaAssocTest on the host: the restatement of DESIGN.md section 20 (tests/assoc_reference.py) against scipy and against
hand-worked numbers, the permutation generator's properties, and the host pieces of hibag_amd/assoc.py (test list, names,
count and percentage columns, argument checks -- all raised before any device work)."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assoc  # noqa: E402


def _tables(rng, rows, below, n):
    out = []
    while len(out) < n:
        t = rng.integers(0, below, (rows, 2))
        if (t.sum(axis=0) > 0).all() and (t.sum(axis=1) > 0).all():
            out.append(t)
    return out


def _close(got, want, rel, absolute=0.0):
    return abs(got - want) <= rel * abs(want) + absolute


# 1 against scipy -------------------------------------------------------------------------------------------------
def test_statistics_against_scipy():
    """2,000 random 2 x 2 tables (Yates) and 3 x 2 tables with cells below 40: 1e-9 relative + 1e-12 absolute.  Measured:
    at most 1.2e-13 relative (2 x 2) and 4.7e-15 (3 x 2)."""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(20)
    worst = [0.0, 0.0]
    for t in _tables(rng, 2, 40, 2000):
        got = float(R.chisq_2x2(int(t.sum()), np.array([t[1, 1]]), np.array([t[1].sum()]), int(t[:, 1].sum()))[0])
        want = float(stats.chi2_contingency(t, correction=True)[0])
        assert _close(got, want, 1e-9, 1e-12), (t, got, want)
        worst[0] = max(worst[0], abs(got - want) / want if want > 1e-3 else 0.0)
    for t in _tables(rng, 3, 40, 2000):
        got = float(R.chisq_3x2(int(t.sum()), int(t[:, 1].sum()), np.array([t[1].sum()]), np.array([t[2].sum()]),
                                np.array([t[1, 1]]), np.array([t[2, 1]]))[0])
        want = float(stats.chi2_contingency(t, correction=False)[0])
        assert _close(got, want, 1e-9, 1e-12), (t, got, want)
        worst[1] = max(worst[1], abs(got - want) / want if want > 1e-3 else 0.0)
    print(f"largest relative difference to scipy: 2 x 2 {worst[0]:.3g}, 3 x 2 {worst[1]:.3g}")


def test_chisq_p_against_scipy():
    """erfc(sqrt(st / 2)) and exp(-st / 2) against chi2.sf for st up to 60.  The tail's relative sensitivity to st is about
    st / 2 <= 30, the special functions on either side are good to a few ulp: about 1e-13; the bound leaves one decade
    (measured: 2.9e-14)."""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(22)
    for st in list(rng.uniform(0, 60, 500)) + [0.0]:
        for df in (1, 2):
            assert _close(R.chisq_p(float(st), df), float(stats.chi2.sf(st, df)), 1e-12), (st, df)
    assert math.isnan(R.chisq_p(math.nan, 1)) and R.chisq_p(0.0, 1) == 1.0 and R.chisq_p(0.0, 2) == 1.0


# ten times the largest relative difference measured on the 500 tables below (1.55e-14: scipy's tie rule uses 1e-14 where
# R's uses 1e-7, and no table of the set has a near-tie in between)
FISHER_BOUND = 1.6e-13


def test_fisher_p_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    assert FISHER_BOUND <= 1e-6
    rng = np.random.default_rng(21)
    worst = 0.0
    for t in _tables(rng, 2, 30, 500):
        got = R.fisher_p(*(int(v) for v in t.ravel()))
        want = float(stats.fisher_exact(t)[1])
        worst = max(worst, abs(got - want) / want)
        assert _close(got, want, FISHER_BOUND), (t, got, want)
    print(f"largest relative difference of fisher_p to scipy: {worst:.3g}")


def test_package_p_values_are_the_restatement():
    """hibag_amd.assoc's own p-value code against the restatement: the same arithmetic, so 1e-15 relative."""
    rng = np.random.default_rng(23)
    tabs = np.zeros((300, 6), np.int64)
    tabs[:, :4] = rng.integers(0, 60, (300, 4))
    tabs[0, :4] = [5, 0, 7, 0]                    # no case: NaN
    tabs[1, :4] = [0, 0, 7, 3]                    # nobody without: NaN
    got = assoc._fisher_p(tabs)
    for t, row in enumerate(tabs[:, :4].tolist()):
        want = R.fisher_p(*row)
        assert (math.isnan(want) and math.isnan(got[t])) or _close(got[t], want, 1e-15), (row, got[t], want)
    assert math.isnan(got[0]) and math.isnan(got[1])
    st = np.concatenate([rng.uniform(0, 80, 200), [0.0, math.nan]])
    for df in (1, 2):
        got = assoc._chisq_p(st, df)
        want = np.array([R.chisq_p(float(s), df) for s in st])
        assert np.array_equal(got, want, equal_nan=True)


# 2 margins -------------------------------------------------------------------------------------------------------
def test_margins():
    N, c1 = 20, 8
    a = np.array([0])
    assert np.isnan(R.chisq_2x2(N, a, np.array([0]), c1)[0])                  # no carrier
    assert np.isnan(R.chisq_2x2(N, np.array([8]), np.array([20]), c1)[0])     # everybody a carrier
    assert np.isnan(R.chisq_2x2(N, a, np.array([5]), 0)[0])                   # no case
    assert np.isnan(R.chisq_2x2(N, np.array([5]), np.array([5]), 20)[0])      # no control
    # D <= 0: |N a - r1 c1| <= N / 2 gives exactly 0.0 (10 carriers, 4 or 5 of 9 cases: det = -10, 10, D = 0; det = 0 below)
    for x, cases in ((4, 9), (5, 9), (4, 8)):
        st = R.chisq_2x2(N, np.array([x]), np.array([10]), cases)[0]
        assert st == 0.0 and not np.signbit(st)
    assert R.chisq_2x2(N, np.array([6]), np.array([10]), 9)[0] > 0
    # 3 x 2: each of the five margins
    ok = dict(N=30, c1=12, r_het=np.array([10]), r_hom=np.array([5]), x_het=np.array([4]), x_hom=np.array([3]))
    assert R.chisq_3x2(**ok)[0] > 0
    for change in (dict(r_het=np.array([0]), x_het=np.array([0])), dict(r_hom=np.array([0]), x_hom=np.array([0])),
                   dict(r_het=np.array([25]), x_het=np.array([9])), dict(c1=0, x_het=np.array([0]), x_hom=np.array([0])),
                   dict(c1=30, x_het=np.array([10]), x_hom=np.array([5]))):
        assert np.isnan(R.chisq_3x2(**dict(ok, **change))[0]), change
    # a worked 2 x 2: 12 samples, 7 carriers, 6 cases, 5 case carriers: D = 2 |60 - 42| - 12 = 24, 24^2 12 / (4 35 36)
    assert R.chisq_2x2(12, np.array([5]), np.array([7]), 6)[0] == (24.0 * 24.0 * 12.0) / ((4.0 * 35.0) * 36.0)


# 3 sampling ------------------------------------------------------------------------------------------------------
def test_every_label_row_has_n_case_ones():
    for n, n_case in ((1, 0), (1, 1), (7, 3), (40, 10), (129, 64), (300, 299)):
        L = R.labels(5, 1, 50, n, n_case)
        assert L.shape == (50, n) and set(np.unique(L)) <= {0, 1}
        assert (L.sum(axis=1) == n_case).all(), (n, n_case)
    assert not R.labels(5, 1, 20, 33, 0).any()
    assert R.labels(5, 1, 20, 33, 33).all()


def test_case_frequencies_are_uniform():
    """4,000 permutations of 40 samples with 10 cases: every sample is a case in 0.25 of them, within 5 standard errors."""
    L = R.labels(2024, 1, 4000, 40, 10)
    freq = L.mean(axis=0)
    se = math.sqrt(0.25 * 0.75 / 4000)
    assert np.abs(freq - 0.25).max() <= 5 * se, freq


def test_rows_differ_and_ranges_split():
    L = R.labels(7, 1, 200, 60, 20)
    assert len({row.tobytes() for row in L}) == 200
    assert np.array_equal(np.concatenate([R.labels(7, 1, 80, 60, 20), R.labels(7, 81, 120, 60, 20)]), L)
    assert not np.array_equal(R.labels(8, 1, 200, 60, 20), L)
    big = (1 << 33) + 5
    assert np.array_equal(R.labels(7, big, 3, 60, 20)[1:], R.labels(7, big + 1, 2, 60, 20))


# 4 the package's host pieces -------------------------------------------------------------------------------------
A, B, Cc = "01:01", "02:01", "03:01"
H1 = [A, A, A, A, B, B, Cc, A, B, A, B, A]
H2 = [A, B, B, Cc, B, Cc, Cc, A, Cc, Cc, B, B]
Y = [1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1]
# worked by hand from the twelve samples: per model the count columns and the percentage of cases, rows A, B, C
WORKED = {
    "dominant": ([[5, 7], [5, 7], [7, 5]], [[20.0, 71.4], [60.0, 42.9], [57.1, 40.0]]),
    "additive": ([[15, 9], [15, 9], [18, 6]], [[33.3, 77.8], [60.0, 33.3], [55.6, 33.3]]),
    "recessive": ([[10, 2], [10, 2], [11, 1]], [[40.0, 100.0], [60.0, 0.0], [54.5, 0.0]]),
    "genotype": ([[5, 5, 2], [5, 5, 2], [7, 4, 1]], [[20.0, 60.0, 100.0], [60.0, 60.0, 0.0], [57.1, 50.0, 0.0]]),
}


def _hla(h1=H1, h2=H2, prob=None):
    return hb.HlaAlleleClass(locus="A", sample_id=[f"s{i}" for i in range(len(h1))], allele1=list(h1), allele2=list(h2), prob=prob)


@pytest.mark.parametrize("model", assoc.MODELS)
def test_hand_worked_columns(model):
    plan = assoc._Plan(_hla(), Y, math.nan, None)
    assert plan.names == [A, B, Cc] and plan.n_samp == 12 and plan.n_case == 6 and plan.n_excluded == 0
    ref = R.Analysis(plan.a1, plan.a2, plan.y, 3, None, model)
    counts, pct = assoc._columns(model, ref.tab)
    want_counts, want_pct = WORKED[model]
    assert counts.tolist() == want_counts
    assert pct.tolist() == want_pct
    assert assoc.COUNT_NAMES[model] == {"dominant": ("[-/-]", "[-/h,h/h]"), "additive": ("[-]", "[h]"),
                                        "recessive": ("[-/-,-/h]", "[h/h]"), "genotype": ("[-/-]", "[-/h]", "[h/h]")}[model]
    empty = np.array([[0, 0, 3, 1, 0, 0]])
    assert np.isnan(assoc._columns(model, empty)[1][0, 0])


def test_test_list_and_names():
    h1, h2 = H1 + [None, "10:01"], H2 + [A, None]            # two samples with an unknown allele: dropped
    y = Y + [1, 0]
    plan = assoc._Plan(_hla(h1, h2), y, math.nan, None)
    assert plan.names == [A, B, Cc] and plan.row == [0, 1, 2] and plan.n_device_tests == 3 and plan.n_samp == 12
    assert plan.group_of is None
    # groups over a longer allele list in another order; "10:01" is carried by a dropped sample only
    alleles = ["10:01", Cc, B, A, "04:01"]
    g = hb.HlaAlleleGroups.from_labels(alleles, "first", ["x", "y", "x", "z", "z"]) + \
        hb.HlaAlleleGroups.from_labels(alleles, "second", ["p", "q", "q", "q", "r"]) + \
        hb.HlaAlleleGroups(alleles, ["third"], [["u", "v", "w"]], np.array([[0, 0, 0, 0, 0]]))
    plan = assoc._Plan(_hla(h1, h2), y, math.nan, g)
    assert plan.names == [A, B, Cc, "first:x", "first:y", "first:z", "second:p", "second:q", "second:r",
                          "third:u", "third:v", "third:w"]
    assert plan.group_of.tolist() == [[2, 0, 1], [1, 1, 1], [0, 0, 0]]
    # the device numbers 0 .. the largest id in use: first 3 levels, second 2 (p carried by nobody, q), third 1
    assert plan.row == [0, 1, 2, 3, 4, 5, 6, 7, -1, 8, -1, -1] and plan.n_device_tests == 9
    # two distinct values of any kind: the smaller is the control
    plan = assoc._Plan(_hla(), ["case" if v else "ctrl" for v in Y], math.nan, None)
    assert plan.y.tolist() == [0 if v else 1 for v in Y]      # "case" < "ctrl"
    assert assoc._Plan(_hla(), [bool(v) for v in Y], math.nan, None).y.tolist() == Y
    assert assoc._Plan(_hla(), np.array(Y, float) * 2 + 1, math.nan, None).y.tolist() == Y
    # the call threshold
    prob = np.array([0.9] * 10 + [0.2, math.nan])
    plan = assoc._Plan(_hla(prob=prob), Y, 0.5, None)
    assert plan.n_excluded == 2 and plan.n_samp == 10 and plan.y.tolist() == Y[:10]


def test_value_errors():
    hla = _hla()
    for bad in (Y[:-1] + [None], Y[:-1] + [math.nan]):
        with pytest.raises(ValueError, match="missing"):
            hb.hlaAssocTest(hla, bad)
    with pytest.raises(ValueError, match="same length"):
        hb.hlaAssocTest(hla, Y[:-1])
    with pytest.raises(ValueError, match="two distinct"):
        hb.hlaAssocTest(hla, [0, 1, 2] * 4)
    with pytest.raises(ValueError, match="two distinct"):
        hb.hlaAssocTest(hla, [5] * 12)
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaAssocTest(hla, Y, model="dominent")
    with pytest.raises(ValueError, match="posterior probability"):
        hb.hlaAssocTest(hla, Y, prob_threshold=0.5)
    with pytest.raises(ValueError, match="n_perm"):
        hb.hlaAssocTest(hla, Y, n_perm=-1)
    with pytest.raises(ValueError, match="seed"):
        hb.hlaAssocTest(hla, Y, n_perm=10, seed=-1)
    g = hb.hlaGroupsByResolution([A, B], "2-digit")
    with pytest.raises(ValueError, match="03:01.*not among the alleles of 'groups'"):
        hb.hlaAssocTest(hla, Y, groups=g)
    with pytest.raises(ValueError, match="no sample"):
        hb.hlaAssocTest(_hla([None] * 12, H2), Y)
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaAssocTest(H1, Y)


# 5 what the association entries share --------------------------------------------------------------------------------
def test_plan_sel_is_the_brute_force_rule():
    """``_Plan.sel``: at or above the threshold (a NaN ``prob`` is excluded), both alleles known, in the original order."""
    h1 = H1 + [None, "10:01", None, A, math.nan]
    h2 = H2 + [A, None, None, B, B]
    y = Y + [1, 0, 1, 0, 1]
    prob = [0.9, 0.2, math.nan, 0.5, 0.7, 0.49, 1.0, 0.8, 0.9, 0.6, 0.2, math.nan, 0.9, 0.9, 0.1, math.nan, 0.9]
    hla = _hla(h1, h2, np.array(prob))
    for thr in (math.nan, math.inf, 0.5, 0.0):
        want = [i for i in range(len(h1))
                if isinstance(h1[i], str) and isinstance(h2[i], str) and (not math.isfinite(thr) or prob[i] >= thr)]
        for labels in (y, None):
            plan = assoc._Plan(hla, labels, thr, None)
            assert plan.sel.tolist() == want and plan.n_samp == len(want), thr
            assert plan.y.tolist() == [y[i] if labels is not None else 0 for i in want]
            assert plan.n_case == sum(plan.y) and plan.y.dtype == np.int32
            assert plan.n_excluded == (sum(1 for p in prob if not p >= thr) if math.isfinite(thr) else 0)


def test_spread_fills_the_levels_unknown_to_the_device():
    """``_Plan.spread``: the device numbers a partition's levels 0 .. the largest id that an allele of the data has, so the
    filled tests are exactly the levels above it -- none of which an allele of the data belongs to; every other test gets its
    device row, whatever the trailing shape."""
    alleles = ["10:01", Cc, B, A, "04:01"]
    labels = {"first": ["x", "y", "x", "z", "z"], "second": ["p", "q", "q", "q", "r"], "third": ["u", "u", "u", "u", "w"]}
    g = hb.HlaAlleleGroups.from_labels(alleles, "first", labels["first"])
    for part in ("second", "third"):
        g = g + hb.HlaAlleleGroups.from_labels(alleles, part, labels[part])
    plan = assoc._Plan(_hla(), Y, math.nan, g)                  # the data has A, B and C only
    filled = []
    for q, part in enumerate(g.names):
        ids = [g.levels[q].index(lab) for a, lab in zip(alleles, labels[part]) if a in plan.alleles]
        filled += [f"{part}:{name}" for lv, name in enumerate(g.levels[q]) if lv > max(ids)]
        assert all(g.levels[q].index(lab) <= max(ids) for a, lab in zip(alleles, labels[part]) if a in plan.alleles)
    assert filled == ["second:r", "third:w"]
    assert [nm for nm, r in zip(plan.names, plan.row) if r < 0] == filled
    T = plan.n_device_tests
    for a in (np.arange(T) + 0.5, np.arange(3 * T, dtype=np.int64).reshape(T, 3), np.arange(4.0 * T).reshape(T, 2, 2)):
        for fill in (np.nan, -7):
            got = plan.spread(a, fill)
            assert got.shape == (len(plan.names),) + a.shape[1:]
            for t, (nm, r) in enumerate(zip(plan.names, plan.row)):
                want = np.full(a.shape[1:], fill) if nm in filled else a[r]
                assert np.array_equal(got[t], want, equal_nan=True), (nm, fill)
    assert plan.spread(np.arange(T), 0).dtype == np.int64


def _raised(entry, *args, **kw):
    with pytest.raises((ValueError, TypeError)) as info:
        entry(*args, **kw)
    return type(info.value), str(info.value)


def test_shared_argument_checks_agree():
    """Every entry that takes one of the shared arguments refuses a bad value with the same exception and message.  (The
    omnibus entries name their own three models, and know partitions beside tests in ``condition``: their messages say so
    and are compared among themselves.)"""
    import assocglm_reference as G
    import assocomni_reference as O
    import assocquant_reference as Q
    hla, y, groups, covar = O.hla_of("n40")
    cov, yq = covar[:, :2], covar[:, 2]
    entries = {
        "test": lambda **kw: hb.hlaAssocTest(hla, y, **kw),
        "glm": lambda covariates=cov, **kw: hb.hlaAssocGlm(hla, y, covariates, _backend=G.Backend, **kw),
        "quant": lambda covariates=cov, **kw: hb.hlaAssocQuant(hla, yq, covariates, _backend=Q.Backend, **kw),
        "omnibus": lambda covariates=cov, **kw: hb.hlaAssocOmnibus(hla, y, groups, covariates, _backend=O.Backend, **kw),
        "stepwise": lambda covariates=cov, **kw: hb.hlaAssocStepwise(hla, y, groups, covariates, _backend=O.Backend, **kw),
    }
    kept = assoc._Plan(hla, y, math.nan, None).sel
    short, holed = cov[:-1], cov.copy()
    holed[kept[3], 1] = math.nan
    regress = ("glm", "quant", "omnibus", "stepwise")
    cases = [
        (dict(model="dominent"), ("test", "glm", "quant"), ValueError, 'should be one of "dominant"'),
        (dict(model="dominent"), ("omnibus", "stepwise"), ValueError, 'should be one of "additive"'),
        (dict(n_perm=-1), ("test", "quant"), ValueError, "n_perm must be an integer >= 0"),
        (dict(n_perm=2.5), ("test", "quant"), ValueError, "n_perm must be an integer >= 0"),
        (dict(n_perm=True), ("test", "quant"), ValueError, "n_perm must be an integer >= 0"),
        (dict(n_perm=3, seed=-1), ("test", "quant"), ValueError, "seed must be an integer in 0 .. 2^64 - 1"),
        (dict(n_perm=3, seed=1 << 64), ("test", "quant"), ValueError, "seed must be an integer in 0 .. 2^64 - 1"),
        (dict(maxit=0), ("glm", "omnibus", "stepwise"), ValueError, "maxit must be an integer >= 1"),
        (dict(maxit=2.0), ("glm", "omnibus", "stepwise"), ValueError, "maxit must be an integer >= 1"),
        (dict(epsilon=0), ("glm", "omnibus", "stepwise"), ValueError, "epsilon must be > 0"),
        (dict(epsilon="small"), ("glm", "omnibus", "stepwise"), ValueError, "epsilon must be > 0"),
        (dict(covariates=short), regress, ValueError, f"covariate 'c1' has {len(y) - 1} values for {len(y)} samples"),
        (dict(covariates=holed), regress, ValueError, "covariate 'c2' has a missing or non-finite value: subset the samples first"),
        (dict(condition=["99:99"]), ("glm", "quant"), ValueError, "condition: '99:99' is not a test of this analysis"),
        (dict(condition=["99:99"]), ("omnibus", "stepwise"), ValueError,
         "condition: '99:99' is neither a partition nor a test of this analysis"),
    ]
    for kw, names, exc, text in cases:
        seen = {name: _raised(entries[name], **kw) for name in names}
        assert len(set(seen.values())) == 1, (kw, seen)
        got_exc, got_text = seen[names[0]]
        assert got_exc is exc and (got_text == text or got_text.startswith("'arg' " + text)), (kw, got_text)
    # a hole in a sample that is not kept is no error
    dropped = sorted(set(range(len(y))) - set(kept.tolist()))
    assert dropped
    holed = cov.copy()
    holed[dropped, :] = math.nan
    assert entries["glm"](covariates=holed).n_samp == len(kept)


def test_assoc_entries_are_declared():
    from hibag_amd import _lib
    for name in ("hibag_hip_assoc_new", "hibag_hip_assoc_free", "hibag_hip_assoc_n_tests", "hibag_hip_assoc_observed",
                 "hibag_hip_assoc_permute", "hibag_hip_assoc_labels"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert "hlaAssocTest" in hb.__all__ and "HlaAssocResult" in hb.__all__
