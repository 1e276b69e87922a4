"""hlaPredictCurve on the GPU: hibag_hip_predict_prefix bit-identical, every sample and every size, to the CPU oracle run on
hlaSubModelObj(obj, size) (tests/curve_reference.py) and to hibag_hip_predict on a device model of that sub-model; the
model's own prediction untouched by a curve call; invalid sizes rejected.  No tolerance anywhere."""
import numpy as np
import pytest

import hibag_amd as hb
from conftest import align_geno
from curve_reference import assert_curve_equal, curve, same_bits
from hibag_amd import NA_INTEGER, synth
from oracle_full import cohort

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def _curve_of(model, G, sizes=None):
    dev = hb.hlaModelFromObj(model)
    try:
        sz = np.arange(1, len(model.classifiers) + 1, dtype=np.int32) if sizes is None else np.asarray(sizes, np.int32)
        got = dev.predict_prefix(G, sz)
        assert dev.status() == 0
        return got
    finally:
        dev.close()


@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_fixture_models_every_size(which, request, hapmap_geno):
    model = request.getfixturevalue(which)
    G = align_geno(model, hapmap_geno)
    assert_curve_equal(_curve_of(model, G), curve(model, G), which)


def test_hla_b_shape_100_classifiers_2048_samples_every_size():
    """Whole groups that miss every SNP of some classifiers, weights that are not powers of two, an all-NA last sample
    (oracle_full's "structured" recipe); the model's own pass 2 is k_accum, so the entry runs on its second layout."""
    model, G, _ = cohort("hla-b", 2048, recipe="structured")
    dev = hb.hlaModelFromObj(model)
    try:
        assert dev.second_pass_pairs() > 0                     # not store mode 1: the lazily built second layout
        got = dev.predict_prefix(G, np.arange(1, 101, dtype=np.int32))
        assert dev.status() == 0 and dev.handover_faults() == 0
    finally:
        dev.close()
    want = curve(model, G)
    assert_curve_equal(got, want, "hla-b")
    assert np.all(got["h1"][:, -1] == NA_INTEGER) and np.all(np.isnan(got["matching"][:, -1]))


@pytest.fixture(scope="module")
def wide_case():
    """One-step FP4, int8, multi-step FP4 and VALU (> 112 SNPs) classifiers; 300 samples (not a multiple of 64), one
    with every SNP missing, some that miss all SNPs of a classifier."""
    counts = [12, 113, 18, 40, 24, 30, 31, 32, 56, 84, 100, 120, 128, 20]
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(counts), snp_counts=counts)
    G, _ = synth.make_samples(founders, af, 300, seed=8)
    G[0, :] = NA_INTEGER
    G[np.ix_(range(64, 80), model.classifiers[0].snpidx)] = NA_INTEGER
    G[np.ix_(range(70, 90), model.classifiers[3].snpidx[1:])] = NA_INTEGER
    return model, G


def test_wide_classifiers_and_a_partial_group(wide_case):
    model, G = wide_case
    assert_curve_equal(_curve_of(model, G), curve(model, G), "wide")


def test_model_that_stores_every_cell_itself():
    """The DRB1 shape stores every cell sum by default (pass 2 = k_accum_cells): the entry runs on the model's own layout."""
    model, founders, af = synth.make_model("hla-drb1", n_classifier=8)
    G, _ = synth.make_samples(founders, af, 200)
    G[7, :] = NA_INTEGER
    dev = hb.hlaModelFromObj(model)
    try:
        assert dev.stored_cells() > 0 and dev.second_pass_pairs() == 0
        before = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        got = dev.predict_prefix(G, np.arange(1, 9, dtype=np.int32))
        after = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        assert dev.status() == 0
    finally:
        dev.close()
    assert_curve_equal(got, curve(model, G), "drb1")
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


def test_several_batches(monkeypatch):
    model, founders, af = synth.make_model("hla-a-small")
    G, _ = synth.make_samples(founders, af, 1000)
    G[999, :] = NA_INTEGER
    G[np.ix_(range(250, 262), model.classifiers[2].snpidx)] = NA_INTEGER
    one = _curve_of(model, G)
    monkeypatch.setenv("HIBAG_PREFIX_BATCH", "256")
    four = _curve_of(model, G)
    want = curve(model, G)
    assert_curve_equal(four, want, "batches of 256")
    assert_curve_equal(one, want, "one batch")


@pytest.mark.parametrize("sizes", [[100], [1], [3, 10, 11, 47, 99]])
def test_size_lists(sizes, model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)
    assert_curve_equal(_curve_of(model_a, G, sizes), curve(model_a, G, sizes), str(sizes))


def test_equal_to_the_library_on_the_sub_model(wide_case, model_oob, hapmap_geno):
    for model, G in (wide_case, (model_oob, align_geno(model_oob, hapmap_geno))):
        sizes = [1, len(model.classifiers) // 2, len(model.classifiers)]
        got = _curve_of(model, G, sizes)
        for i, k in enumerate(sizes):
            sub = hb.hlaModelFromObj(hb.hlaSubModelObj(model, k))
            try:
                r = sub.predict_raw(G, 1, want_dosage=False)
            finally:
                sub.close()
            assert np.array_equal(got["h1"][i], r["h1"]) and np.array_equal(got["h2"][i], r["h2"]), k
            assert same_bits(got["prob"][i], r["prob"]) and same_bits(got["matching"][i], r["matching"]), k


def test_the_models_own_prediction_is_untouched(model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)
    dev = hb.hlaModelFromObj(model_a)
    try:
        stored, pairs = dev.stored_cells(), dev.second_pass_pairs()
        before = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        dev.predict_prefix(G, [5, 50])
        dev.predict_prefix(G, [100])
        after = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        assert dev.status() == 0 and (dev.stored_cells(), dev.second_pass_pairs()) == (stored, pairs)
    finally:
        dev.close()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
        if before[k].dtype.kind == "f":
            assert same_bits(before[k], after[k]), k


@pytest.mark.parametrize("sizes", [[0, 1], [1, 101], [2, 2], [5, 3], []])
def test_invalid_sizes(sizes, model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    dev = hb.hlaModelFromObj(model_a)
    try:
        with pytest.raises(hb.HibagHipError) as e:
            dev.predict_prefix(G, np.asarray(sizes, np.int32))
        assert e.value.code == -1 and "sizes" in str(e.value)
        assert dev.status() == 0
    finally:
        dev.close()


def test_hla_predict_curve_end_to_end(model_a, hapmap_geno):
    """The public function on an hlaSNPGenoClass (hlaPredict's SNP matching) with true types."""
    ids = list(hapmap_geno.sample_id)[:40]
    snp = hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(40)))
    res = hb.hlaPredictCurve(model_a, snp, sizes=[1, 10, 100], match_type="RefSNP", verbose=False)
    G = align_geno(model_a, hapmap_geno, ids)
    want = curve(model_a, G, [1, 10, 100])
    got = {"h1": np.stack([p.h1 for p in res.pred]), "h2": np.stack([p.h2 for p in res.pred]),
           "prob": np.stack([p.prob for p in res.pred]), "matching": np.stack([p.matching for p in res.pred])}
    assert_curve_equal(got, want, "hlaPredictCurve")
    assert res.changed[-1] == 0 and res.pred[0].sample_id == ids and res.accuracy is None
    dev = hb.hlaModelFromObj(model_a)
    try:
        ref = hb.hlaPredict(dev, snp, type="response", match_type="RefSNP", verbose=False)
        again = hb.hlaPredictCurve(dev, snp, sizes=[100], hla=ref, match_type="RefSNP", verbose=False)
    finally:
        dev.close()
    assert np.array_equal(again.pred[0].h1, ref.h1) and same_bits(again.pred[0].prob, ref.prob)
    assert again.accuracy[0] == 1.0
