"""hlaPredictCurve on the host: the numpy / oracle restatement of the curve (tests/curve_reference.py) checked against the
oracle on the full model, and the parts of hlaPredictCurve that need no device -- argument checks, the `sizes` default,
`changed` and `accuracy` assembled from given arrays (hibag_amd.curve.curve_from_arrays)."""
import numpy as np
import pytest

import hibag_amd as hb
from conftest import align_geno
from curve_reference import curve, same_bits
from hibag_amd import NA_INTEGER
from hibag_amd.curve import curve_from_arrays, curve_sizes


def test_reference_curve_ends_at_the_full_model(model_a, hapmap_geno, oracle):
    G = align_geno(model_a, hapmap_geno)[:20]
    ref = curve(model_a, G, [1, 50, 100], avx2=False)
    full = oracle.predict(oracle.flatten(model_a), G, vote_method=1, want_prob=False)
    for k in ("h1", "h2"):
        assert np.array_equal(ref[k][2], full[k])
    assert same_bits(ref["prob"][2], full["prob"]) and same_bits(ref["matching"][2], full["matching"])
    # a one-classifier model's SNP weights are all 1: another prediction than the full model's first term
    one = oracle.predict(oracle.flatten(hb.hlaSubModelObj(model_a, 1)), G, vote_method=1, want_prob=False)
    assert same_bits(ref["prob"][0], one["prob"]) and not same_bits(ref["prob"][0], ref["prob"][2])
    assert same_bits(curve(model_a, G, [50])["prob"][0], ref["prob"][1])          # the AVX2 port agrees


def test_sizes_default_and_checks():
    assert np.array_equal(curve_sizes(None, 5), [1, 2, 3, 4, 5]) and curve_sizes(None, 5).dtype == np.int32
    assert np.array_equal(curve_sizes([2, 5], 5), [2, 5])
    assert np.array_equal(curve_sizes(np.array([1.0, 3.0]), 5), [1, 3])
    for bad in ([], [0, 1], [1, 6], [2, 2], [3, 2], [1.5], [[1, 2]], ["a"]):
        with pytest.raises(ValueError):
            curve_sizes(bad, 5)
    with pytest.raises(ValueError):
        curve_sizes(None, 0)


def _arrays():
    NA = NA_INTEGER
    #            s0  s1  s2  s3
    h1 = np.array([[0, 1, NA, 2],       # size 1
                   [0, 0, 0, 2],        # size 2
                   [0, 0, 0, 1]], np.int32)
    h2 = np.array([[1, 1, NA, 2],
                   [1, 2, 1, 2],
                   [1, 2, 1, 2]], np.int32)
    prob = np.array([[.5, .4, 0., .9], [.6, .5, .3, .8], [.7, .6, .4, .5]])
    return h1, h2, prob, prob * 0.5


def test_changed_and_accuracy_from_arrays(model_a):
    h1, h2, prob, mt = _arrays()
    ids = ["a", "b", "c", "d"]
    al = model_a.hla_allele
    res = curve_from_arrays(model_a, [1, 2, 3], ids, h1, h2, prob, mt, assembly="hg19")
    assert np.array_equal(res.sizes, [1, 2, 3]) and np.array_equal(res.changed, [3, 1, 0])
    assert res.accuracy is None and len(res.pred) == 3
    p = res.pred[0]
    assert isinstance(p, hb.HlaAlleleClass) and p.sample_id == ids and p.assembly == "hg19" and p.locus == model_a.hla_locus
    assert p.allele1 == [al[0], al[1], None, al[2]] and p.allele2 == [al[1], al[1], None, al[2]]
    assert np.array_equal(p.prob, prob[0]) and np.array_equal(p.matching, mt[0]) and p.dosage is None and p.postprob is None
    true = hb.HlaAlleleClass(locus=model_a.hla_locus, sample_id=ids, allele1=[al[0], al[0], al[0], al[1]],
                             allele2=[al[1], al[2], al[1], al[2]])
    res = curve_from_arrays(model_a, [1, 2, 3], ids, h1, h2, prob, mt, hla=true)
    want = [hb.hlaCompareAllele(true, q)["acc.haplo"] for q in res.pred]
    assert np.array_equal(res.accuracy, want) and np.array_equal(res.accuracy, [3 / 6, 7 / 8, 1.0])
    assert [o["total.num.ind"] for o in res.overall] == [3, 4, 4]


def test_changed_ignores_the_order_of_a_pair(model_a):
    h1 = np.array([[1, 0], [0, 0]], np.int32)
    h2 = np.array([[0, 1], [1, 1]], np.int32)
    z = np.zeros((2, 2))
    assert np.array_equal(curve_from_arrays(model_a, [1, 2], ["a", "b"], h1, h2, z, z).changed, [0, 0])


def test_arrays_of_the_wrong_shape(model_a):
    h1, h2, prob, mt = _arrays()
    with pytest.raises(ValueError):
        curve_from_arrays(model_a, [1, 2], ["a", "b", "c", "d"], h1, h2, prob, mt)


def test_argument_checks_before_any_device_work(model_a):
    G = np.zeros((model_a.n_snp, 3), np.int32)
    with pytest.raises(TypeError):
        hb.hlaPredictCurve("model", G)
    with pytest.raises(ValueError):
        hb.hlaPredictCurve(model_a, G, sizes=[3, 2], verbose=False)
    with pytest.raises(ValueError):
        hb.hlaPredictCurve(model_a, G, sizes=[101], verbose=False)
    with pytest.raises(TypeError):
        hb.hlaPredictCurve(model_a, G, hla="truth", verbose=False)
