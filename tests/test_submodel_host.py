"""hlaSubModelObj and hlaCombineModelObj (R/HIBAG.R:1121-1129, :1069-1114) on the host."""
import dataclasses

import numpy as np
import pytest

import hibag_amd as hb
from conftest import align_geno
from curve_reference import first_classifiers, same_bits
from hibag_amd import rdata

FIELDS = [f.name for f in dataclasses.fields(hb.HlaAttrBagObj) if f.name != "classifiers"]


def test_submodel_is_the_first_n_classifiers(model_a):
    sub = hb.hlaSubModelObj(model_a, 7)
    assert len(sub.classifiers) == 7 and all(a is b for a, b in zip(sub.classifiers, model_a.classifiers))
    for f in FIELDS:
        assert getattr(sub, f) is getattr(model_a, f), f
    assert len(model_a.classifiers) == 100                      # the argument is not modified
    ref = first_classifiers(model_a, 7)
    assert all(a is b for a, b in zip(sub.classifiers, ref.classifiers)) and len(ref.classifiers) == 7


def test_submodel_of_every_classifier_predicts_like_the_model(model_a, hapmap_geno, oracle):
    G = align_geno(model_a, hapmap_geno)
    full = oracle.predict(oracle.flatten(model_a), G, vote_method=1)
    sub = oracle.predict(oracle.flatten(hb.hlaSubModelObj(model_a, len(model_a.classifiers))), G, vote_method=1)
    for k in ("h1", "h2"):
        assert np.array_equal(full[k], sub[k])
    for k in ("prob", "matching", "dosage", "postprob"):
        assert same_bits(full[k], sub[k]), k


@pytest.mark.parametrize("n", [0, -1, 101, 1.5])
def test_submodel_rejects_sizes_outside_the_model(model_a, n):
    with pytest.raises(ValueError):
        hb.hlaSubModelObj(model_a, n)


def test_submodel_rejects_other_types(model_a):
    with pytest.raises(TypeError):
        hb.hlaSubModelObj(model_a, "3")
    with pytest.raises(TypeError):
        hb.hlaSubModelObj({"classifiers": []}, 1)


def _rest(model, k):
    return dataclasses.replace(model, classifiers=list(model.classifiers[k:]))


def test_combine_gives_the_classifiers_back_in_order(model_oob):
    both = hb.hlaCombineModelObj(hb.hlaSubModelObj(model_oob, 37), _rest(model_oob, 37))
    assert len(both.classifiers) == 100 and all(a is b for a, b in zip(both.classifiers, model_oob.classifiers))
    assert both.sample_id == list(model_oob.sample_id) and both.n_samp == model_oob.n_samp
    assert both.snp_id == list(model_oob.snp_id) and both.hla_allele == list(model_oob.hla_allele)
    assert both.appendix is None
    # identical sample.id: the weighted mean, in the reference's operation order
    m = np.asarray(model_oob.matching, np.float64)
    assert same_bits(both.matching, 37 / 100 * m + 63 / 100 * m)
    # frequency means: (a + a) * 0.5 is a again
    assert same_bits(both.snp_allele_freq, model_oob.snp_allele_freq) and same_bits(both.hla_freq, model_oob.hla_freq)


def test_combine_matching_concatenated_for_different_samples(model_oob):
    a = hb.hlaSubModelObj(model_oob, 10)
    ids = [s + "x" for s in model_oob.sample_id[:5]] + list(model_oob.sample_id[5:])
    b = dataclasses.replace(_rest(model_oob, 90), sample_id=ids, matching=np.asarray(model_oob.matching) * 0.5)
    both = hb.hlaCombineModelObj(a, b)
    assert same_bits(both.matching, np.concatenate([model_oob.matching, np.asarray(model_oob.matching) * 0.5]))
    assert both.sample_id == list(model_oob.sample_id) + ids[:5] and both.n_samp == len(model_oob.sample_id) + 5
    assert len(both.classifiers) == 20


def test_combine_frequency_means_and_appendix(model_oob):
    a = dataclasses.replace(hb.hlaSubModelObj(model_oob, 3),
                            appendix=rdata.RList([rdata.RStrings(["Illumina"]), rdata.RStrings(["note"])],
                                                 {"names": ["platform", "information"]}))
    fa, fh = np.asarray(model_oob.snp_allele_freq) * 0.25, np.asarray(model_oob.hla_freq)[::-1].copy()
    b = dataclasses.replace(_rest(model_oob, 98), snp_allele_freq=fa, hla_freq=fh,
                            appendix=rdata.RList([rdata.RStrings(["Illumina", "Affymetrix"]), rdata.RStrings(["careful"])],
                                                 {"names": ["platform", "warning"]}))
    both = hb.hlaCombineModelObj(a, b)
    assert same_bits(both.snp_allele_freq, (np.asarray(model_oob.snp_allele_freq) + fa) * 0.5)
    assert same_bits(both.hla_freq, (np.asarray(model_oob.hla_freq) + fh) * 0.5)
    assert list(both.appendix["platform"]) == ["Illumina", "Affymetrix"]
    assert list(both.appendix["information"]) == ["note"] and list(both.appendix["warning"]) == ["careful"]


@pytest.mark.parametrize("field,value", [("hla_locus", "B"), ("assembly", "hg18"), ("snp_id", None), ("hla_allele", None)])
def test_combine_stops_on_a_mismatch(model_oob, field, value):
    if value is None:
        value = list(getattr(model_oob, field))[:-1] + ["other"]
    other = dataclasses.replace(model_oob, **{field: value})
    with pytest.raises(ValueError, match="identical"):
        hb.hlaCombineModelObj(model_oob, other)
    with pytest.raises(TypeError):
        hb.hlaCombineModelObj(model_oob, None)


def test_combined_model_survives_a_round_trip(model_oob, tmp_path, hapmap_geno, oracle):
    both = hb.hlaCombineModelObj(hb.hlaSubModelObj(model_oob, 60), _rest(model_oob, 60))
    path = str(tmp_path / "combined.RData")
    hb.save_model(path, both)
    back = hb.load_model(path, "mobj")
    assert len(back.classifiers) == 100 and back.sample_id == both.sample_id and back.hla_allele == both.hla_allele
    assert same_bits(back.matching, both.matching) and same_bits(back.hla_freq, both.hla_freq)
    for x, y in zip(back.classifiers, model_oob.classifiers):
        assert np.array_equal(x.snpidx, y.snpidx) and same_bits(x.freq, y.freq) and x.haplo == y.haplo
        assert np.array_equal(x.hla, y.hla) and np.array_equal(x.samp_num, y.samp_num)
    G = align_geno(model_oob, hapmap_geno)
    a = oracle.predict(oracle.flatten(back), G, vote_method=1, want_prob=False)
    b = oracle.predict(oracle.flatten(model_oob), G, vote_method=1, want_prob=False)
    assert np.array_equal(a["h1"], b["h1"]) and same_bits(a["prob"], b["prob"])
