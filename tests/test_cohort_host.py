"""The resident cohort without a device: the numpy statement of the resident form (tests/cohort_reference.py), the
argument checks of hlaPredictLoci (raised before the library is touched) and load_model_list."""
import os

import numpy as np
import pytest

import hibag_amd as hb
from cohort_reference import NA, allele_freq, canonical, codes, counts, pack, random_geno, stride_of, unpack
from conftest import REFDATA
from hibag_amd import _lib, synth
from hibag_amd.snpmatch import _row_afreq

SIZES = [1, 3, 4, 63, 64, 65, 1000]


@pytest.mark.parametrize("n_samp", SIZES)
@pytest.mark.parametrize("snp_major", [True, False])
def test_pack_unpack_is_the_identity(n_samp, snp_major):
    rng = np.random.default_rng(n_samp)
    g = random_geno(rng, 7, n_samp)
    src = np.ascontiguousarray(g if snp_major else g.T)
    rows = pack(src, snp_major)
    assert rows.shape == (7, stride_of(n_samp)) and rows.dtype == np.uint8 and stride_of(n_samp) % 16 == 0
    assert 4 * stride_of(n_samp) >= n_samp
    assert np.array_equal(unpack(rows, n_samp), canonical(g))
    assert np.all(codes(rows)[:, n_samp:] == 1), "the slots behind the last sample read as missing"


@pytest.mark.parametrize("n_samp", [5, 64, 333])
def test_pack_equals_the_payload_of_a_bed_file(n_samp, tmp_path):
    rng = np.random.default_rng(3)
    g = canonical(random_geno(rng, 11, n_samp))
    path = synth.write_bed(str(tmp_path / "c.bed"), np.ascontiguousarray(g.T))
    raw = np.fromfile(path, np.uint8)
    assert list(raw[:3]) == [0x6C, 0x1B, 1]
    w = (n_samp + 3) // 4
    payload = raw[3:].reshape(11, w)
    rows = pack(g)
    full = n_samp // 4
    assert np.array_equal(rows[:, :full], payload[:, :full])
    if n_samp % 4:
        keep = (1 << (2 * (n_samp % 4))) - 1                  # the file's last byte, as far as it holds samples
        assert np.array_equal(rows[:, full] & keep, payload[:, full] & keep)
        rest = 0xFF ^ keep
        assert np.all((rows[:, full] & rest) == (0x55 & rest))
    assert np.all(rows[:, w:] == 0x55)
    assert np.array_equal(unpack(rows, n_samp), g)


@pytest.mark.parametrize("n_samp", [1, 63, 65, 1000])
def test_counts_and_frequencies_equal_row_afreq(n_samp):
    rng = np.random.default_rng(100 + n_samp)
    g = canonical(random_geno(rng, 9, n_samp))
    g[4, :] = NA                                               # a SNP nobody is called at: NaN
    rows = pack(g)
    n_valid, total = counts(rows)
    assert n_valid.dtype == np.int32 and total.dtype == np.int64
    assert np.array_equal(n_valid, (g != NA).sum(axis=1))
    assert np.array_equal(total, np.where(g != NA, g, 0).sum(axis=1))
    assert np.array_equal(allele_freq(rows), _row_afreq(g), equal_nan=True)
    assert np.isnan(allele_freq(rows)[4])


def _obj(locus, seed=1):
    m, founders, af = synth.make_model("hla-a-small", seed=seed, n_classifier=3)
    m.hla_locus = locus
    return m, founders, af


def test_predict_loci_argument_errors_come_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    a, founders, af = _obj("A")
    b, _, _ = _obj("B", seed=2)
    G, _ = synth.make_samples(founders, af, 8)
    snp = synth.as_snp_geno(a, G)
    with pytest.raises(ValueError, match="more than once"):
        hb.hlaPredictLoci([a, _obj("A", seed=5)[0]], snp, verbose=False)
    with pytest.raises(ValueError, match="empty"):
        hb.hlaPredictLoci([], snp, verbose=False)
    with pytest.raises(ValueError, match="empty"):
        hb.hlaPredictLoci({}, snp, verbose=False)
    with pytest.raises(TypeError, match="every element"):
        hb.hlaPredictLoci({"A": a, "B": "not a model"}, snp, verbose=False)
    with pytest.raises(TypeError):
        hb.hlaPredictLoci(a, snp, verbose=False)
    with pytest.raises(ValueError, match="'arg' should be one of"):
        hb.hlaPredictLoci([a, b], snp, type="dosage", verbose=False)
    with pytest.raises(ValueError, match="'arg' should be one of"):
        hb.hlaPredictLoci([a, b], snp, vote="mean", verbose=False)
    with pytest.raises(TypeError, match="'snp' must be"):
        hb.hlaPredictLoci([a, b], G, verbose=False)
    with pytest.raises(TypeError, match="'snp' must be"):
        hb.HlaDeviceCohort(G)
    with pytest.raises(ValueError, match="snp_sel"):
        hb.HlaDeviceCohort(snp, snp_sel=[0, a.n_snp])


def test_load_model_list():
    path = os.path.join(REFDATA, "ModelList.RData")
    lst = hb.load_model_list(path, "modellist")
    assert list(lst) == ["A"]
    one = hb.load_model(path, "modellist", "A")
    got = lst["A"]
    assert isinstance(got, hb.HlaAttrBagObj)
    assert got.hla_locus == one.hla_locus and got.hla_allele == one.hla_allele and got.snp_id == one.snp_id
    assert got.n_snp == one.n_snp and got.n_samp == one.n_samp and got.assembly == one.assembly
    assert np.array_equal(got.snp_position, one.snp_position) and got.snp_allele == one.snp_allele
    assert len(got.classifiers) == len(one.classifiers)
    for x, y in zip(got.classifiers, one.classifiers):
        assert np.array_equal(x.snpidx, y.snpidx) and np.array_equal(x.freq, y.freq) and np.array_equal(x.hla, y.hla)
        assert x.haplo == y.haplo
    assert hb.load_model_list(path).keys() == lst.keys()
    with pytest.raises(ValueError, match="list of models"):
        hb.load_model_list(os.path.join(REFDATA, "OutOfBag.RData"), "mobj")
