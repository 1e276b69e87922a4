"""hlaAssocTest on the GPU: the label rows of hibag_hip_assoc_labels equal the restatement (tests/assoc_reference.py: DESIGN.md
section 20 in numpy) byte for byte; the observed tables are equal as integers and the statistics, the per-permutation maxima
and the counts bit for bit, per model, at the tile edges of the Gram, whatever the panel size and however the permutations
are split over calls; hlaAssocTest's table equals the restatement's; invalid arguments are rejected."""
import warnings

import numpy as np
import pytest

import hibag_amd as hb
import assoc_reference as R
from hibag_amd import NA_INTEGER, _lib, assoc, synth

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
MODELS = assoc.MODELS
SEED = (1 << 40) + 3


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = bits(got) == bits(want)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.flatnonzero(~(same | both_nan))
    assert bad.size == 0, f"{what}: {bad.size} entries differ, the first at {bad[0]}: got {got[bad[0]]!r}, reference {want[bad[0]]!r}"


# 1 labels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_labels_equal_the_restatement(n):
    zeros = np.zeros(n, np.int32)
    for n_case in sorted({0, 1, n // 2, n}):
        y = np.zeros(n, np.int32)
        y[np.random.default_rng(n + n_case).choice(n, n_case, replace=False)] = 1
        with assoc._DeviceAssoc(zeros, zeros, y, 1, None, 0) as dev:
            for seed in (1, SEED):
                for perm0 in (1, 1 << 33):
                    got = dev.labels(seed, perm0, 70)                 # (two wavefronts, the second partial)
                    want = R.labels(seed, perm0, 70, n, n_case)
                    assert got.dtype == np.int8 and got.shape == (70, n)
                    assert np.array_equal(got.view(np.uint8), want), (n, n_case, seed, perm0)
                    assert (got.sum(axis=1) == n_case).all()


def test_labels_across_panels(monkeypatch):
    """70 rows in panels of 64 and 6: each panel reaches the host before the next overwrites the device's buffer."""
    n, n_case = 300, 150
    zeros, y = np.zeros(n, np.int32), np.zeros(n, np.int32)
    y[np.random.default_rng(n + n_case).choice(n, n_case, replace=False)] = 1
    monkeypatch.setenv("HIBAG_ASSOC_PANEL_PERMS", "64")
    with assoc._DeviceAssoc(zeros, zeros, y, 1, None, 0) as dev:
        for perm0 in (1, 1 << 33):
            assert dev.labels(SEED, perm0, 70).tobytes() == R.labels(SEED, perm0, 70, n, n_case).tobytes(), perm0


def test_labels_skip_the_dropped_samples():
    a1 = np.array([0, NA, 1, 0, 1, NA], np.int32)
    a2 = np.array([0, 1, NA, 1, 1, NA], np.int32)
    y = np.array([1, 1, 1, 0, 1, 0], np.int32)
    with assoc._DeviceAssoc(a1, a2, y, 2, None, 0) as dev:
        assert dev.n_kept == 3
        assert np.array_equal(dev.labels(9, 1, 10).view(np.uint8), R.labels(9, 1, 10, 3, 2))


# 2 statistics and counts -----------------------------------------------------------------------------------------
def cohort(n_allele, n_samp=300, seed=0):
    """300 samples over n_allele alleles with a skewed frequency, some homozygous, 5 % with an unknown allele; two
    partitions, the first with a level (id 1) that no allele has; labels associated with allele 0."""
    rng = np.random.default_rng(1000 * n_allele + seed)
    w = 1.0 / np.arange(1, n_allele + 1) ** 0.7
    a = rng.choice(n_allele, (n_samp, 2), p=w / w.sum()).astype(np.int32)
    hom = rng.random(n_samp) < 0.15
    a[hom, 1] = a[hom, 0]
    y = (rng.random(n_samp) < np.where((a == 0).any(axis=1), 0.7, 0.3)).astype(np.int32)
    a[rng.random((n_samp, 2)) < 0.05] = NA
    g = np.stack([np.where(np.arange(n_allele) % 3 == 0, 0, 2 + np.arange(n_allele) % 5), np.arange(n_allele) // 7]).astype(np.int32)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), y, g


@pytest.fixture(scope="module")
def references():
    """Per (model, n_allele): the cohort, the restatement's analysis and its 200 permutations' statistics, made once."""
    cache = {}

    def get(model, n_allele):
        key = (model, n_allele)
        if key not in cache:
            a1, a2, y, g = cohort(n_allele)
            A = R.Analysis(a1, a2, y, n_allele, g, model)
            cache[key] = (a1, a2, y, g, A, A.permute(SEED, 1, 200))
        return cache[key]
    return get


@pytest.mark.parametrize("n_allele", [63, 64, 65])
@pytest.mark.parametrize("model", MODELS)
def test_observed_and_permuted_equal_the_restatement(model, n_allele, references, monkeypatch):
    a1, a2, y, g, A, (want_max, want_count) = references(model, n_allele)
    assert (a1 == NA).any() and (a1 == a2).any() and not A.tab[n_allele + 1, 2:].any()        # unknown, homozygous, the empty level
    with assoc._DeviceAssoc(a1, a2, y, n_allele, g, MODELS.index(model)) as dev:
        assert dev.n_tests == A.n_tests and dev.n_kept == A.n
        stat, table = dev.observed()
        assert np.array_equal(table, A.tab), model
        assert_bits(stat, A.stat, f"{model} observed")
        assert np.isnan(stat[n_allele + 1]) and np.isfinite(stat[0]) and np.nanmax(stat) > 0
        got_max, got_count = dev.permute(SEED, 1, 200)
        assert_bits(got_max, want_max, f"{model} max_stat")
        assert np.array_equal(got_count, want_count), model
        assert got_count[n_allele + 1] == 0 and got_count.max() > 0
        for n in (1, 63, 64, 65):
            m, c = dev.permute(SEED, 1, n)
            w_max, w_count = A.permute(SEED, 1, n)
            assert_bits(m, w_max, f"{model} max_stat of {n}")
            assert np.array_equal(c, w_count), (model, n)
            assert_bits(m, want_max[:n], f"{model} a prefix")
        # the panel size shows nowhere
        monkeypatch.setenv("HIBAG_ASSOC_PANEL_PERMS", "64")
        m, c = dev.permute(SEED, 1, 200)
        monkeypatch.delenv("HIBAG_ASSOC_PANEL_PERMS")
        assert_bits(m, got_max, f"{model} panels of 64")
        assert np.array_equal(c, got_count)
        # two calls of 100 against one of 200
        m1, c1 = dev.permute(SEED, 1, 100)
        m2, c2 = dev.permute(SEED, 101, 100)
        assert_bits(np.concatenate([m1, m2]), got_max, f"{model} split")
        assert np.array_equal(c1 + c2, got_count)
        m0, c0 = dev.permute(SEED, 1, 0)
        assert m0.size == 0 and not c0.any()


# 3 end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_hla_assoc_test_equals_the_restatement(model):
    """The tests' spread case (14 alleles, half the genotypes missing) predicted on the device, a phenotype enriched in the
    carriers of the most frequent predicted allele, a call threshold, two-digit groups plus a partition with levels the data
    do not reach."""
    mobj, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.5)
    G[77, :] = NA
    hb.hlaSetKernelTarget("hip")
    dev = hb.hlaModelFromObj(mobj)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            hla = hb.hlaPredict(dev, synth.as_snp_geno(mobj, G), type="response", verbose=False)
    finally:
        dev.close()
    h1, h2 = list(hla.allele1), list(hla.allele2)
    thr = 0.05
    ok = [i for i in range(130) if h1[i] is not None and h2[i] is not None and hla.prob[i] >= thr]
    names = hb.hlaUniqueAllele([h1[i] for i in ok] + [h2[i] for i in ok])
    carried = [sum((h1[i] == a) or (h2[i] == a) for i in ok) for a in names]
    planted = int(np.argmax(carried))
    rng = np.random.default_rng(5)
    carrier = np.array([h1[i] == names[planted] or h2[i] == names[planted] for i in range(130)])
    y = (rng.random(130) < np.where(carrier, 0.9, 0.15)).astype(int)
    alleles = list(mobj.hla_allele)
    groups = hb.hlaGroupsByResolution(alleles, "2-digit") + \
        hb.HlaAlleleGroups(alleles, ["tail"], [["in", "gap", "out", "beyond"]], np.array([[0 if a in names else 2 for a in alleles]]))
    res = hb.hlaAssocTest(hla, y, model=model, prob_threshold=thr, groups=groups, n_perm=999, seed=77)
    assert res.n_excluded == int(np.sum(~(np.asarray(hla.prob) >= thr))) and res.n_samp == len(ok) and res.seed == 77

    # the restatement on the same kept samples; its tests are the levels 0 .. the largest id among the data's alleles
    pos = {a: i for i, a in enumerate(names)}
    a1 = np.array([pos[h1[i]] for i in ok]); a2 = np.array([pos[h2[i]] for i in ok])
    g = groups.group_of[:, [alleles.index(a) for a in names]]
    want = R.assoc_test(a1, a2, y[ok], len(names), g, model, n_perm=999, seed=77)
    rows, want_names = list(range(len(names))), list(names)
    nxt = len(names)
    for q in range(groups.n_part):
        top = int(g[q].max()) + 1
        for lv, name in enumerate(groups.levels[q]):
            want_names.append(f"{groups.names[q]}:{name}")
            rows.append(nxt + lv if lv < top else -1)
        nxt += top
    assert res.name == want_names and rows[-3:] == [-1, -1, -1]
    rows = np.array(rows)
    known = rows >= 0
    tab = res.to_table()
    k = len(res.count_names)
    assert list(tab)[:2 * k] == list(res.count_names) + ["%." + c for c in res.count_names]
    assert list(tab)[2 * k:] == ["chisq.st", "chisq.p", "fisher.p", "perm.p", "perm.p.adj"]
    assert np.array_equal(res.counts[known], want["counts"][rows[known]])
    assert np.array_equal(res.pct[known], want["pct"][rows[known]], equal_nan=True)
    assert_bits(res.chisq_st[known], want["chisq_st"][rows[known]], "chisq_st")
    assert_bits(res.max_stat, want["max_stat"], "max_stat")
    for key in ("chisq_p", "fisher_p", "perm_p", "perm_p_adj"):
        got, ref = getattr(res, key)[known], want[key][rows[known]]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), key
        fin = ~np.isnan(ref)
        assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-15 * np.abs(ref[fin])), key
    # the levels the data do not reach: everybody without, NaN statistics
    unit = 2 if model == "additive" else 1
    assert (res.counts[~known, 0] == unit * len(ok)).all() and not res.counts[~known, 1:].any()
    for key in ("chisq_st", "chisq_p", "fisher_p", "perm_p", "perm_p_adj"):
        assert np.isnan(getattr(res, key)[~known]).all(), key
    if model == "genotype":
        assert np.isnan(res.fisher_p).all()
    fin = ~np.isnan(res.perm_p)
    assert fin.any() and (res.perm_p_adj[fin] >= res.perm_p[fin]).all()
    if model in ("dominant", "additive"):           # (the other two rest on the few homozygotes among 130 samples)
        assert res.perm_p_adj[planted] == np.nanmin(res.perm_p_adj) and res.perm_p_adj[planted] <= 0.01


# 4 errors --------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    a = np.zeros(4, np.int32)
    y = np.array([0, 1, 0, 1], np.int32)
    p = assoc._ptr

    def refused(*args):
        h = L.hibag_hip_assoc_new(*args)
        msg = L.hibag_hip_last_error().decode()
        assert not h and msg.startswith("hibag_hip_assoc_new"), msg
        return msg

    refused(None, p(a), p(y), 4, 1, None, 0, 0)
    refused(p(a), None, p(y), 4, 1, None, 0, 0)
    refused(p(a), p(a), None, 4, 1, None, 0, 0)
    refused(p(a), p(a), p(y), 4, 1, None, 1, 0)
    assert "2^24" in refused(p(a), p(a), p(y), (1 << 24) + 1, 1, None, 0, 0)
    assert "model" in refused(p(a), p(a), p(y), 4, 1, None, 0, 4)
    assert "model" in refused(p(a), p(a), p(y), 4, 1, None, 0, -1)
    assert "tests" in refused(p(a), p(a), p(y), 4, 40000, None, 0, 0)
    assert "allele index" in refused(p(np.array([0, 1, 0, 0], np.int32)), p(a), p(y), 4, 1, None, 0, 0)
    assert "label" in refused(p(a), p(a), p(np.array([0, 1, 2, 1], np.int32)), 4, 1, None, 0, 0)
    with assoc._DeviceAssoc(a, a, y, 1, None, 0) as dev:
        stat = np.empty(1)
        table = np.empty((1, 6), np.int64)
        count = np.empty(1, np.int64)
        einval = -1
        assert L.hibag_hip_assoc_observed(dev._h, None, p(table)) == einval and L.hibag_hip_last_error()
        assert L.hibag_hip_assoc_observed(None, p(stat), p(table)) == einval
        assert L.hibag_hip_assoc_permute(dev._h, 1, 1, 5, None, p(count)) == einval
        assert L.hibag_hip_assoc_permute(dev._h, 1, 1, 5, p(np.empty(5)), None) == einval
        assert L.hibag_hip_assoc_permute(dev._h, 1, 0, 5, p(np.empty(5)), p(count)) == einval      # permutation 0 is the observed one
        assert L.hibag_hip_assoc_permute(None, 1, 1, 5, p(np.empty(5)), p(count)) == einval
        assert L.hibag_hip_assoc_labels(dev._h, 1, 1, 3, None) == einval
        assert L.hibag_hip_assoc_labels(dev._h, 1, 0, 3, p(np.empty((3, 4), np.int8))) == einval
        assert L.hibag_hip_assoc_n_tests(None) == einval
        assert b"hibag_hip_assoc" in L.hibag_hip_last_error()
