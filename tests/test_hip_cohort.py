"""The resident cohort on the GPU: HlaDeviceCohort, hlaPredictLoci and the C entries hibag_hip_cohort_* /
hibag_hip_predict[_topk]_cohort.  The contract is equality with the routes that take the raw genotypes on every call:
every comparison here is exact (NaN == NaN), there is no tolerance in this feature; after every call the model's status
is 0 and no hand-over fault was counted.

BED files: the HapMap CEU fixture (SNP-major) and, written by conftest.write_bed, a SNP-major and an individual-major
file of a synthetic cohort -- both storage modes are covered."""
import os
import warnings

import numpy as np
import pytest

import hibag_amd as hb
from cohort_reference import canonical, counts, pack, random_geno
from conftest import REFDATA, write_bed
from hibag_amd import NA_INTEGER, synth
from hibag_amd.hibag import _TYPES, _VOTES

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def clean(m):
    assert m.status() == 0 and m.handover_faults() == 0


def assert_same(got, want, what):
    """Two results of hlaPredict (an HlaAlleleClass, or the posterior matrix of type="prob"), field by field."""
    if isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == want.dtype, what
        assert np.array_equal(got, want, equal_nan=True), what
        return
    assert got.locus == want.locus and got.sample_id == want.sample_id and got.assembly == want.assembly, what
    assert np.array_equal(got.h1, want.h1) and np.array_equal(got.h2, want.h2), what
    assert got.allele1 == want.allele1 and got.allele2 == want.allele2, what
    assert np.array_equal(got.prob, want.prob, equal_nan=True) and np.array_equal(got.matching, want.matching, equal_nan=True), what
    assert got.pair_names == want.pair_names, what
    for f in ("dosage", "postprob"):
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), f"{what}: {f}"
        if b is not None:
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: {f}"


def assert_same_top(got, want, what):
    for f in ("h1", "h2"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f"{what}: {f}"
    for f in ("prob", "matching"):
        assert np.array_equal(getattr(got, f), getattr(want, f), equal_nan=True), f"{what}: {f}"
    assert got.k == want.k and got.locus == want.locus and got.sample_id == want.sample_id and got.assembly == want.assembly, what


def assert_raw_equal(got, want, what, rows=slice(None)):
    assert set(got) == set(want), what
    for k in want:
        assert np.array_equal(got[k], want[k][rows], equal_nan=True), f"{what}: {k}"


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samp", [1, 63, 65, 1000, 3001])
@pytest.mark.parametrize("order", ["C", "F"])
def test_snp_counts_equal_numpy(n_samp, order):
    check_counts(n_samp, 137, order)


@pytest.mark.parametrize("n_samp,n_snp,order", [(10_007, 523, "F"),      # R's order, several slabs along the samples
                                                (300, 9_001, "F"),       # ... and along the SNPs (more than 8,192 per slab)
                                                (300_001, 12, "C")])     # numpy's order, rows cut at 2^18 samples
def test_snp_counts_across_slabs(n_samp, n_snp, order):
    check_counts(n_samp, n_snp, order)


def check_counts(n_samp, n_snp, order):
    rng = np.random.default_rng(n_samp)
    g = random_geno(rng, n_snp, n_samp)
    g[7, :] = NA
    snp = hb.HlaSNPGeno(genotype=np.asarray(g, order=order), sample_id=[f"s{i}" for i in range(n_samp)],
                        snp_id=[f"rs{i}" for i in range(n_snp)], snp_position=np.arange(n_snp, dtype=np.float64),
                        snp_allele=["A/G"] * n_snp, assembly="hg19")
    want_n, want_sum = counts(pack(g))
    c = canonical(g)
    assert np.array_equal(want_n, (c != NA).sum(axis=1)) and np.array_equal(want_sum, np.where(c != NA, c, 0).sum(axis=1))
    with hb.HlaDeviceCohort(snp) as coh:
        assert coh.n_samp == n_samp and coh.n_snp == n_snp and coh.nbytes == n_snp * (((n_samp + 3) // 4 + 15) // 16 * 16)
        n_valid, total = coh.snp_counts()
        assert n_valid.dtype == np.int32 and total.dtype == np.int64
        assert np.array_equal(n_valid, want_n) and np.array_equal(total, want_sum)
        from hibag_amd.snpmatch import _row_afreq
        rows = np.array([0, 7, 5, n_snp - 1])
        assert np.array_equal(coh.allele_freq(rows), _row_afreq(c[rows]), equal_nan=True)
    sel = rng.permutation(n_snp)[:min(50, n_snp)]
    with hb.HlaDeviceCohort(snp, snp_sel=sel) as coh:
        assert coh.n_snp == len(sel) and coh.snp_id == [snp.snp_id[i] for i in sel]
        n_valid, total = coh.snp_counts()
        assert np.array_equal(n_valid, want_n[sel]) and np.array_equal(total, want_sum[sel])


# 2 ---------------------------------------------------------------------------------------------------------------
def three_loci(n_samp=3000):
    """Three models of different shapes on disjoint SNP sets and ONE cohort whose SNPs are a shuffled superset of most of
    theirs: a tenth of every model's SNPs absent, a third with reversed alleles, strand-ambiguous SNPs that the allele
    frequencies decide, missing genotypes, one sample without a single genotype, and SNPs no model knows."""
    specs = [("A", "hla-a-small", dict(wide_classifier=False, seed=21)),                       # classifiers of at most 30 SNPs
             ("W", "hla-a-small", dict(n_snp=150, n_classifier=6, snp_counts=[40, 64, 100, 113, 120, 128], seed=22)),
             ("B", "hla-b", dict(seed=23))]                                                       # the default HLA-B shape
    rng = np.random.default_rng(5)
    models, rows, ids, pos, alle = {}, [], [], [], []
    for li, (locus, shape, kw) in enumerate(specs):
        model, founders, af = synth.make_model(shape, **kw)
        model.hla_locus = locus
        model.snp_position = model.snp_position + 1_000_000 * li
        model.snp_id = [f"{locus}_{s}" for s in model.snp_id]
        S = model.n_snp
        amb = rng.random(S) < 0.15
        model.snp_allele = ["C/G" if a else "A/G" for a in amb]
        G, _ = synth.make_samples(founders, af, n_samp, seed=40 + li)
        G[5, :] = NA
        keep = rng.random(S) < 0.9
        flip = rng.random(S) < 0.33
        for j in np.where(keep)[0]:
            g = G[:, j].copy()
            if flip[j] and not amb[j]:
                g = np.where(g == NA, NA, 2 - g)
            rows.append(g); ids.append(model.snp_id[j]); pos.append(model.snp_position[j])
            alle.append("C/G" if amb[j] else ("G/A" if flip[j] else "A/G"))
        assert (flip & keep & ~amb).any() and (amb & keep).any() and not keep.all()
        models[locus] = model
    for e in range(40):
        rows.append(rng.integers(0, 3, n_samp).astype(np.int32)); ids.append(f"x{e}"); pos.append(1000.0 + e); alle.append("C/T")
    order = rng.permutation(len(rows))
    snp = hb.HlaSNPGeno(genotype=np.array([rows[i] for i in order], np.int32), sample_id=[f"s{i}" for i in range(n_samp)],
                        snp_id=[ids[i] for i in order], snp_position=np.array([pos[i] for i in order], np.float64),
                        snp_allele=[alle[i] for i in order], assembly="hg19")
    return models, snp


@pytest.fixture(scope="module")
def loci_case():
    models, snp = three_loci()
    dev = {k: hb.hlaModelFromObj(m) for k, m in models.items()}
    yield models, dev, snp
    for m in dev.values():
        m.close()


@pytest.mark.parametrize("vote", _VOTES)
@pytest.mark.parametrize("type_", _TYPES)
def test_predict_loci_equals_the_loop(loci_case, type_, vote):
    models, dev, snp = loci_case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("No prediction output for 1 individual": sample 5)
        loop = {k: hb.hlaPredict(m, snp, type=type_, vote=vote, verbose=False) for k, m in dev.items()}
        got = hb.hlaPredictLoci(dev, snp, type=type_, vote=vote, verbose=False)
        assert list(got) == list(dev)
        for k in dev:
            assert_same(got[k], loop[k], f"fresh cohort, {k} {type_} {vote}")
            clean(dev[k])
        with hb.HlaDeviceCohort(snp) as coh:     # one resident cohort, all three models, both entries
            res = hb.hlaPredictLoci(list(dev.values()), coh, type=type_, vote=vote, verbose=False)
            assert list(res) == list(dev)
            for k, m in dev.items():
                assert_same(res[k], loop[k], f"resident cohort through hlaPredictLoci, {k} {type_} {vote}")
                assert_same(hb.hlaPredict(m, coh, type=type_, vote=vote, verbose=False), loop[k], f"hlaPredict on the cohort, {k}")
                clean(m)


def test_predict_loci_other_sources_and_topk(loci_case, capsys):
    models, dev, snp = loci_case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loop = {k: hb.hlaPredict(m, snp, type="response+prob", verbose=False) for k, m in dev.items()}
        # R's memory order of the same matrix; host objects in place of device models; verbose output per locus
        snp_f = hb.HlaSNPGeno(genotype=np.asfortranarray(snp.genotype), sample_id=snp.sample_id, snp_id=snp.snp_id,
                              snp_position=snp.snp_position, snp_allele=snp.snp_allele, assembly=snp.assembly)
        got = hb.hlaPredictLoci(models, snp_f, type="response+prob", verbose=False)
        for k in models:
            assert_same(got[k], loop[k], f"Fortran order, HlaAttrBagObj, {k}")
        capsys.readouterr()
        got = hb.hlaPredictLoci(dev, snp, type="response+prob", verbose=True)
        text = capsys.readouterr().out
        for k in dev:
            assert_same(got[k], loop[k], f"verbose, {k}")
            assert f"HIBAG model for HLA-{k}:" in text
        assert text.count("# of samples: 3000") == 3 and text.count("Matching the SNPs between the model and the test data:") == 3
        with hb.HlaDeviceCohort(snp_f) as coh:
            for k, m in dev.items():
                assert_same(hb.hlaPredict(m, coh, type="response+prob", verbose=False), loop[k], f"cohort from Fortran order, {k}")
                for vote in _VOTES:
                    want = hb.hlaPredictTopK(m, snp, k=3, vote=vote, verbose=False)
                    assert_same_top(hb.hlaPredictTopK(m, coh, k=3, vote=vote, verbose=False), want, f"top-k, {k} {vote}")
                    clean(m)
            with pytest.raises(ValueError, match="cl"):
                hb.hlaPredict(dev["A"], coh, cl=[0], verbose=False)


def test_stray_values_decide_alike_whatever_verbose(loci_case, capsys):
    """Values outside 0..2 that are not NA (3, -1) on strand-ambiguous SNPs: hlaPredict's strand check adds them up on
    the host matrix.  hlaPredictLoci on that host object consults the same frequencies, printing or not."""
    models, dev, snp = loci_case
    g = np.array(snp.genotype, np.int32)
    amb = np.array([a == "C/G" for a in snp.snp_allele])
    rng = np.random.default_rng(17)
    stray = amb[:, None] & (rng.random(g.shape) < 0.4)
    g[stray] = np.where(rng.random(int(stray.sum())) < 0.7, 3, -1)
    bad = hb.HlaSNPGeno(genotype=g, sample_id=snp.sample_id, snp_id=snp.snp_id, snp_position=snp.snp_position,
                        snp_allele=snp.snp_allele, assembly=snp.assembly)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loop = {k: hb.hlaPredict(m, bad, type="response+prob", verbose=False) for k, m in dev.items()}
        for verbose in (False, True):
            got = hb.hlaPredictLoci(dev, bad, type="response+prob", verbose=verbose)
            capsys.readouterr()
            for k in dev:
                assert_same(got[k], loop[k], f"stray values, verbose={verbose}, {k}")
                clean(dev[k])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_sample_windows_and_a_cohort_larger_than_a_batch():
    model, founders, af = synth.make_model("hla-a-small", seed=3)
    dev = hb.hlaModelFromObj(model)
    try:
        n = dev.batch_limit() + 3000 + 17
        G, _ = synth.make_samples(founders, af, n, seed=31)
        G[n - 1, :] = NA
        S = model.n_snp
        rng = np.random.default_rng(8)
        perm = rng.permutation(S + 9)                       # cohort row of model SNP k: perm[k]; nine rows nobody uses
        col = perm[:S].astype(np.int32).copy()
        col[[3, 40]] = -1
        flip = (rng.random(S) < 0.3)
        mat = np.zeros((S + 9, n), np.int32)
        mat[perm[:S]] = G.T
        snp = hb.HlaSNPGeno(genotype=mat, sample_id=[str(i) for i in range(n)], snp_id=[f"r{i}" for i in range(S + 9)],
                            snp_position=np.arange(S + 9, dtype=np.float64), snp_allele=["A/G"] * (S + 9), assembly="hg19")
        want = dev.predict_mapped(np.ascontiguousarray(mat.T), col, flip, 1, want_dosage=True, want_prob=True)
        clean(dev)
        with hb.HlaDeviceCohort(snp) as coh:
            whole = dev.predict_cohort(coh, col, flip, 1, want_dosage=True, want_prob=True)
            clean(dev)
            assert_raw_equal(whole, want, "larger than a batch: predict_cohort against predict_mapped")
            for first, count in ((0, n), (1, 1), (63, 66), (n - 1, 1)):
                part = dev.predict_cohort(coh, col, flip, 1, want_dosage=True, want_prob=True, first=first, count=count)
                clean(dev)
                assert_raw_equal(part, whole, f"window ({first}, {count})", slice(first, first + count))
            top = dev.predict_topk_cohort(coh, col, flip, 4, 2, first=63, count=66)
            ref = dev.predict_topk_mapped(np.ascontiguousarray(mat.T[63:129]), col, flip, 4, 2)
            clean(dev)
            assert_raw_equal(top, ref, "top-k window")
    finally:
        dev.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_hapmap_bed_through_a_cohort(which, request):
    model = request.getfixturevalue(which)
    lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
    loaded = lazy.load()
    m = hb.hlaModelFromObj(model)
    try:
        with hb.HlaDeviceCohort(lazy) as coh:
            assert coh.n_samp == len(lazy.sample_id) and coh.n_snp == len(lazy.snp_id)
            for vote in _VOTES:
                kw = dict(type="response+prob", vote=vote, match_type="RefSNP", verbose=False)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = hb.hlaPredict(m, coh, **kw)
                    clean(m)
                    assert_same(got, hb.hlaPredict(m, lazy, **kw), f"{which}: cohort from the file against the lazy BED route")
                    assert_same(got, hb.hlaPredict(m, loaded, **kw), f"{which}: cohort from the file against the loaded genotypes")
                    assert_same(hb.hlaPredictLoci([m], lazy, **kw)[model.hla_locus], got, f"{which}: hlaPredictLoci on the lazy file")
                    clean(m)
    finally:
        m.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_synthetic_bed_both_storage_modes(mode, tmp_path):
    from hibag_amd.bed import HlaBEDGeno
    model, founders, af = synth.make_model("hla-a-small", seed=6)
    n = 1003
    G, _ = synth.make_samples(founders, af, n, seed=61)
    G[2, :] = NA
    rng = np.random.default_rng(4)
    perm = rng.permutation(model.n_snp)                    # the file holds the model's SNPs in another order
    path = write_bed(str(tmp_path / "c.bed"), G.T[perm], mode)
    bed = HlaBEDGeno(bed_fn=path, mode=mode, n_bed_samp=n, n_bed_snp=model.n_snp, bed_index=np.arange(model.n_snp, dtype=np.int64),
                     sample_id=[f"S{i}" for i in range(n)], snp_id=[model.snp_id[i] for i in perm],
                     snp_position=np.asarray(model.snp_position)[perm], snp_allele=[model.snp_allele[i] for i in perm],
                     assembly=model.assembly)
    snp = hb.HlaSNPGeno(genotype=np.ascontiguousarray(G.T[perm]), sample_id=bed.sample_id, snp_id=bed.snp_id,
                        snp_position=bed.snp_position, snp_allele=bed.snp_allele, assembly=bed.assembly)
    m = hb.hlaModelFromObj(model)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = hb.hlaPredict(m, snp, type="response+prob", verbose=False)
            with hb.HlaDeviceCohort(bed) as coh, hb.HlaDeviceCohort(snp) as coh2:
                n1, s1 = coh.snp_counts()
                n2, s2 = coh2.snp_counts()
                assert np.array_equal(n1, n2) and np.array_equal(s1, s2)
                assert_same(hb.hlaPredict(m, coh, type="response+prob", verbose=False), want, f"BED mode {mode}")
                clean(m)
            with hb.HlaDeviceCohort(bed, snp_sel=np.arange(0, model.n_snp, 2)) as half:
                sub = hb.HlaSNPGeno(genotype=snp.genotype[::2], sample_id=snp.sample_id, snp_id=snp.snp_id[::2],
                                    snp_position=snp.snp_position[::2], snp_allele=snp.snp_allele[::2], assembly=snp.assembly)
                assert_same(hb.hlaPredict(m, half, verbose=False), hb.hlaPredict(m, sub, verbose=False), f"BED mode {mode}, every other SNP")
                clean(m)
    finally:
        m.close()
    short = str(tmp_path / "short.bed")
    with open(path, "rb") as f, open(short, "wb") as o:
        o.write(f.read()[:-5])
    bed.bed_fn = short
    with pytest.raises(hb.HibagHipError, match="holds fewer than"):
        hb.HlaDeviceCohort(bed)
    bed.bed_fn = str(tmp_path / "none.bed")
    with pytest.raises(hb.HibagHipError, match="Fail to open the file"):
        hb.HlaDeviceCohort(bed)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_the_models_own_prediction_is_untouched(loci_case):
    models, dev, snp = loci_case
    model, m = models["B"], dev["B"]
    _, founders, af = synth.make_model("hla-b", seed=23)
    G, _ = synth.make_samples(founders, af, 2048, seed=77)
    before = {v: m.predict_raw(G, v, want_dosage=True, want_prob=True) for v in (1, 2)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with hb.HlaDeviceCohort(snp) as coh:
            for vote in _VOTES:
                hb.hlaPredict(m, coh, type="response+prob", vote=vote, verbose=False)
                hb.hlaPredictTopK(m, coh, k=5, vote=vote, verbose=False)
        hb.hlaPredictLoci(dev, snp, verbose=False)
    for v in (1, 2):
        assert_raw_equal(m.predict_raw(G, v, want_dosage=True, want_prob=True), before[v], f"predict_raw after the cohort calls, vote {v}")
    clean(m)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_rejections():
    model, founders, af = synth.make_model("hla-a-small", seed=9)
    G, _ = synth.make_samples(founders, af, 200, seed=91)
    snp = synth.as_snp_geno(model, G)
    m = hb.hlaModelFromObj(model)
    try:
        coh = hb.HlaDeviceCohort(snp)
        col = np.arange(model.n_snp, dtype=np.int32)
        good = m.predict_cohort(coh, col)
        for first, count in ((-1, 10), (0, 201), (200, 1), (150, 51), (0, -1)):
            with pytest.raises(hb.HibagHipError, match="outside the cohort") as e:
                m.predict_cohort(coh, col, first=first, count=count)
            assert e.value.code == -1
        bad = col.copy()
        bad[17] = model.n_snp
        with pytest.raises(hb.HibagHipError, match=r"snp_col\[17\]") as e:
            m.predict_cohort(coh, bad)
        assert e.value.code == -1
        with pytest.raises(hb.HibagHipError, match=r"snp_col\[17\]"):
            m.predict_topk_cohort(coh, bad, None, 3)
        with pytest.raises(ValueError):
            m.predict_topk_cohort(coh, col, None, 0)
        assert_raw_equal(m.predict_cohort(coh, col), good, "after the rejected calls")
        clean(m)
        coh.close()
        coh.close()                                       # closing twice is harmless
        for call in (lambda: hb.hlaPredict(m, coh, verbose=False), lambda: hb.hlaPredictTopK(m, coh, verbose=False),
                     lambda: hb.hlaPredictLoci([m], coh, verbose=False), lambda: m.predict_cohort(coh, col),
                     lambda: coh.allele_freq([0]), lambda: coh.snp_counts(), lambda: coh.nbytes):
            with pytest.raises(ValueError, match="closed"):
                call()
    finally:
        m.close()


def test_a_model_on_another_device_is_rejected():
    if hb._lib.lib().hibag_hip_device_count() < 2:
        pytest.skip("needs two devices")
    model, founders, af = synth.make_model("hla-a-small", seed=9)
    G, _ = synth.make_samples(founders, af, 100, seed=91)
    L = hb._lib.lib()
    try:
        with hb.HlaDeviceCohort(synth.as_snp_geno(model, G), device=0) as coh:
            other = hb.hlaModelFromObj(model, device=1)
            try:
                with pytest.raises(hb.HibagHipError, match="on device") as e:
                    other.predict_cohort(coh, np.arange(model.n_snp, dtype=np.int32))
                assert e.value.code == -1
                with pytest.raises(hb.HibagHipError, match="on device"):
                    hb.hlaPredict(other, coh, verbose=False)
            finally:
                other.close()
    finally:
        L.hibag_hip_set_device(0)
