"""hlaDistance on the host: the vectorised CPU reference (tests/distance_reference.py) against a literal transliteration
of HIBAG_Distance and R's fold, bit for bit; the argument checks that fail before any device work; the new C entries."""

import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, synth  # noqa: E402


def same_bits(a, b):
    """Equal values and NaN positions, and the same 64 bits wherever not NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a[keep].view(np.uint64), b[keep].view(np.uint64))


def small_models():
    """Synthetic models small enough for the literal loop: word edges of the packed haplotypes, an allele without
    haplotypes, alleles missing from some classifiers, a one-haplotype classifier, underflowing frequency products."""
    out = {}
    m, _, _ = synth.make_model("hla-a-small", seed=3, n_classifier=6, n_haplo=30, snp_counts=[1, 63, 64, 65, 127, 128], n_snp=140)
    out["snp-widths"] = m
    m, _, _ = synth.make_model("hla-a-small", seed=4, n_classifier=4, n_haplo=25)
    for c in m.classifiers:                                     # allele 0 nowhere, allele 1 only in classifier 0
        keep = (c.hla != 0) & ((c.hla != 1) | (c is m.classifiers[0]))
        c.hla, c.freq, c.haplo = c.hla[keep], c.freq[keep], [h for h, k in zip(c.haplo, keep) if k]
    out["absent-alleles"] = m
    m, _, _ = synth.make_model("hla-a-small", seed=5, n_classifier=3, n_haplo=20)
    c = m.classifiers[1]
    m.classifiers[1] = dataclasses.replace(c, hla=c.hla[:1], freq=np.array([1.0]), haplo=c.haplo[:1])
    out["one-haplotype"] = m
    m, _, _ = synth.make_model("hla-a-small", seed=6, n_classifier=3, n_haplo=20)
    for c in m.classifiers[:2]:
        c.freq = c.freq.copy()
        c.freq[c.hla == c.hla[0]] = 1e-200                      # products 1e-400: 0, a cell of 0/0
    out["underflow"] = m
    return out


@pytest.mark.parametrize("name", ["snp-widths", "absent-alleles", "one-haplotype", "underflow"])
def test_reference_equals_literal_on_synthetic_models(name):
    model = small_models()[name]
    got, got_each = R.distance(model)
    want, want_each = R.literal_distance(model)
    assert same_bits(got_each, want_each)
    assert same_bits(got, want)
    if name == "absent-alleles":
        assert np.isnan(got[0]).all() and np.isnan(got[:, 0]).all()
    if name == "underflow":
        c0 = model.classifiers[0]
        a = int(c0.hla[0])
        assert np.isnan(got_each[0, a, a]) and np.isnan(got_each[1, a, a])


def test_reference_equals_literal_on_the_fixture_models(model_a, model_oob):
    for model in (model_a, model_oob):
        got, got_each = R.distance(model)
        want, want_each = R.literal_distance(model)
        assert same_bits(got_each, want_each)
        assert same_bits(got, want)
        assert np.isfinite(np.diagonal(got)).any() and (np.nan_to_num(np.diagonal(got)) >= 0).all()


def test_cumsum_is_the_reference_order_and_sum_is_not():
    """The reason the reference uses cumsum: a pairwise sum gives other bits on the same data."""
    rng = np.random.default_rng(1)
    v = rng.gamma(0.5, 1.0, 4000) * rng.integers(0, 30, 4000)
    seq = 0.0
    for x in v:
        seq += x
    assert np.cumsum(v)[-1] == seq
    assert np.sum(v) != seq


def test_argument_errors():
    model, _, _ = synth.make_model("hla-a-small", seed=3, n_classifier=2)
    with pytest.raises(TypeError, match="hlaAttrBagObj"):
        hb.hlaDistance("model")
    with pytest.raises(TypeError, match="classifiers"):
        hb.hlaDistance(model, classifiers="yes")
    with pytest.raises(ValueError, match="no classifier"):
        hb.hlaDistance(dataclasses.replace(model, classifiers=[]))
    c = model.classifiers[0]
    bad = dataclasses.replace(c, hla=c.hla[::-1].copy(), freq=c.freq[::-1].copy(), haplo=c.haplo[::-1])
    with pytest.raises(hb.HibagHipError, match="grouped by ascending HLA allele"):
        hb.hlaDistance(dataclasses.replace(model, classifiers=[bad]))


def test_c_entry_rejects_null_and_empty_models():
    L = _lib.lib()
    out = np.empty((3, 3))
    assert L.hibag_hip_model_distance(None, out.ctypes.data_as(C.c_void_p), None) == -1
    m = C.c_void_p(L.hibag_hip_model_new(3, 10))
    try:
        assert L.hibag_hip_model_distance(m, None, None) == -1
        assert L.hibag_hip_model_distance(m, out.ctypes.data_as(C.c_void_p), None) == -1
        assert b"no classifier" in L.hibag_hip_last_error()
    finally:
        L.hibag_hip_model_free(m)
    ms = C.c_double(-1)
    assert L.hibag_hip_model_distance_ms(None, C.byref(ms)) == -1


def test_distance_symbols_are_exported():
    L = _lib.lib()
    for s in ("hibag_hip_model_distance", "hibag_hip_model_distance_ms"):
        assert s in _lib.EXPORTS
        assert hasattr(L, s)
    assert "hlaDistance" in hb.__all__ and hb.hlaDistance is not None
