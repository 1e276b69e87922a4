"""hlaDistance on the GPU: hibag_hip_model_distance bit-identical to the CPU restatement of HIBAG_Distance and R's fold
(tests/distance_reference.py), the result and every classifier's matrix, on the fixture models, the benchmark shapes and
the edge cases; and predictions on the same model unchanged by it."""

import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as R  # noqa: E402
from test_distance_host import same_bits, small_models  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(model, dev=None):
    """hlaDistance of the HlaAttrBagObj, and of the HlaAttrBagClass if given, against the reference."""
    want, want_each = R.distance(model)
    got, got_each = hb.hlaDistance(model, classifiers=True)
    bad = [c for c in range(len(model.classifiers)) if not same_bits(got_each[c], want_each[c])]
    assert not bad, f"classifiers {bad[:10]} differ"
    assert same_bits(got, want)
    assert same_bits(hb.hlaDistance(model), want)
    if dev is not None:
        g2, e2 = hb.hlaDistance(dev, classifiers=True)
        assert same_bits(g2, got) and same_bits(e2, got_each)
    return got


def test_fixture_models(model_a, model_oob):
    for model in (model_a, model_oob):
        dev = hb.hlaModelFromObj(model)
        got = _check(model, dev)
        assert got.shape == (model.n_hla, model.n_hla)
        dev.close()


@pytest.mark.parametrize("shape", ["hla-a-small", "hla-b", "hla-drb1"])
def test_benchmark_shapes(shape):
    model, _, _ = synth.make_model(shape)
    big = max(max(np.bincount(c.hla)) for c in model.classifiers)
    if shape == "hla-drb1":
        assert big * (big + 1) // 2 > 64 * 64                  # cells of many 64-pair chunks on one wave
    _check(model)


@pytest.mark.parametrize("name", ["snp-widths", "absent-alleles", "one-haplotype", "underflow"])
def test_edge_models(name):
    model = small_models()[name]
    got = _check(model)
    if name == "absent-alleles":
        assert np.isnan(got[0]).all() and np.isnan(got[:, 0]).all()
        assert not np.isnan(got[1, 1])                         # allele 1: one classifier only, num = 1


def test_one_classifier_and_one_allele():
    model, _, _ = synth.make_model("hla-b", seed=11, n_classifier=1)
    _check(model)
    model, _, _ = synth.make_model("hla-a-small", seed=12, n_hla=1, n_classifier=5, n_haplo=30)
    got = _check(model)
    assert got.shape == (1, 1) and np.isfinite(got[0, 0])


def test_large_cells_and_wide_classifiers():
    """Alleles with up to hundreds of haplotypes: diagonal cells of ~10^5 pairs, rectangles of ~10^4."""
    model, _, _ = synth.make_model("hla-drb1", seed=13, n_hla=6, n_classifier=4, n_haplo=1200,
                                   snp_counts=[128, 65, 64, 7])
    _check(model)


def test_chunked_fold(monkeypatch):
    """Classifiers in chunks of 7 (the fold carried from chunk to chunk) give the same bits."""
    model, _, _ = synth.make_model("hla-b", seed=14, n_classifier=23)
    want = hb.hlaDistance(model, classifiers=True)
    monkeypatch.setenv("HIBAG_DIST_CHUNK", "7")
    got = hb.hlaDistance(model, classifiers=True)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    _check(model)


def test_adding_a_classifier_after_a_distance():
    """On a model that was never finalized the haplotype table is built by the distance call and rebuilt after an add."""
    model, _, _ = synth.make_model("hla-a-small", seed=15, n_classifier=4)
    L = _lib.lib()
    h = C.c_void_p(L.hibag_hip_model_new(model.n_hla, model.n_snp))
    n = model.n_hla
    out = np.empty((n, n))
    try:
        for k, c in enumerate(model.classifiers):
            strs = (C.c_char_p * len(c.haplo))(*[s.encode() for s in c.haplo])
            _lib.check(L.hibag_hip_model_add_classifier(h, len(c.snpidx), c.snpidx.ctypes.data_as(C.c_void_p), len(c.freq),
                                                        c.freq.ctypes.data_as(C.c_void_p), c.hla.ctypes.data_as(C.c_void_p), strs))
            _lib.check(L.hibag_hip_model_distance(h, out.ctypes.data_as(C.c_void_p), None))
            want, _ = R.distance(dataclasses.replace(model, classifiers=model.classifiers[:k + 1]))
            assert same_bits(out, want), f"after classifier {k}"
        ms = C.c_double(-1)
        _lib.check(L.hibag_hip_model_distance_ms(h, C.byref(ms)))
        assert ms.value >= 0
    finally:
        L.hibag_hip_model_free(h)


def test_predictions_unchanged_around_a_distance():
    model, founders, af = synth.make_model("hla-b", seed=16, n_classifier=12)
    G, _ = synth.make_samples(founders, af, 200, seed=17)
    rng = np.random.default_rng(18)
    samp_num = np.stack([np.bincount(rng.integers(0, 200, 200), minlength=200) for _ in model.classifiers]).astype(np.int32)

    ref = hb.hlaModelFromObj(model)
    p0 = ref.predict_raw(G, vote_method=1, want_dosage=True, want_prob=True)
    o0 = ref.predict_oob(G, samp_num)
    ref.close()

    dev = hb.hlaModelFromObj(model)
    d0 = hb.hlaDistance(dev)
    p1 = dev.predict_raw(G, vote_method=1, want_dosage=True, want_prob=True)
    d1 = hb.hlaDistance(dev)
    o1 = dev.predict_oob(G, samp_num)
    d2 = hb.hlaDistance(dev)
    p2 = dev.predict_raw(G, vote_method=1, want_dosage=True, want_prob=True)
    dev.close()
    for k in p0:
        assert np.array_equal(p0[k], p1[k], equal_nan=True) and np.array_equal(p0[k], p2[k], equal_nan=True), k
    for k in o0:
        assert np.array_equal(o0[k], o1[k], equal_nan=True), k
    want, _ = R.distance(model)
    assert same_bits(d0, want) and same_bits(d1, want) and same_bits(d2, want)
