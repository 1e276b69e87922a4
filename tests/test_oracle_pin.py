"""Pins the CPU oracle against outputs the reference itself produced.

The reference's own tests hold no golden posteriors.  What
the reference does ship are two pre-fit models whose stored fields are outputs
of the hot path (tests/test_ref_pin.py runs the reference's code itself):

* ``outofbag.acc`` of every classifier = 0.5 * (#correct alleles) / #OOB, with
  the count coming from ``_BestGuess`` over the out-of-bag samples
  (src/LibHLA.cpp:1934-1955, :2121).  2 models x 100 classifiers.
* ``matching`` of OutOfBag.RData = ``hlaPredict()$value$matching`` on the 34
  training samples (R/HIBAG.R:253-258), i.e. the weighted mean over classifiers
  of the pre-normalisation posterior total returned by ``_PostProb2``.

Genotypes come from data/HapMap_CEU_Geno.rdata and true alleles from
data/HLA_Type_Table.rdata (both copied as fixtures under tests/golden/).
"""

import numpy as np
import pytest

from conftest import align_geno


def _truth(model, table):
    ti = {s: i for i, s in enumerate(table["sample.id"])}
    lut = {a: i for i, a in enumerate(model.hla_allele)}
    a1 = [lut[table["A.1"][ti[s]]] for s in model.sample_id]
    a2 = [lut[table["A.2"][ti[s]]] for s in model.sample_id]
    return a1, a2


@pytest.mark.parametrize("which", ["oob", "a"])
def test_outofbag_accuracy_of_every_classifier(which, oracle, hapmap_geno, hla_type_table, model_oob, model_a):
    model = model_oob if which == "oob" else model_a
    fm = oracle.flatten(model)
    G = align_geno(model, hapmap_geno)
    a1, a2 = _truth(model, hla_type_table)
    assert len(model.classifiers) == 100
    for c, cl in enumerate(model.classifiers):
        oob = np.where(cl.samp_num == 0)[0]
        assert len(oob) > 0
        correct = 0
        for s in oob:
            s1, s2 = oracle.int_to_snp(G[s], cl.snpidx)
            p1, p2 = oracle.best_guess(fm, c, s1, s2)
            correct += oracle.compare_hla(p1, p2, a1[s], a2[s])
        assert 0.5 * correct / len(oob) == cl.outofbag_acc, f"classifier {c}"


def test_matching_vector_bit_exact(oracle, hapmap_geno, model_oob):
    model = model_oob
    fm = oracle.flatten(model)
    G = align_geno(model, hapmap_geno)
    out = oracle.predict(fm, G, vote_method=1)
    complete = np.array([np.all((g >= 0) & (g <= 2)) for g in G])
    assert complete.sum() == 27
    # every sample without missing SNPs reproduces the stored double exactly
    assert np.array_equal(out["matching"][complete], model.matching[complete])

    # The 7 samples with missing SNPs were written by an older release whose
    # ensemble step was an unweighted mean over ALL classifiers of the totals of
    # the classifiers that see at least one typed SNP.  The per-classifier
    # totals (the hot loop's output) still reproduce the stored doubles exactly.
    for i in np.where(~complete)[0]:
        acc = 0.0
        for c, cl in enumerate(model.classifiers):
            g = G[i][cl.snpidx]
            if not np.any((g >= 0) & (g <= 2)):
                continue
            s1, s2 = oracle.int_to_snp(G[i], cl.snpidx)
            acc += oracle.post_prob2(fm, c, s1, s2)[1]
        assert acc / len(model.classifiers) == model.matching[i], f"sample {i}"


def test_training_set_calls(oracle, hapmap_geno, hla_type_table, model_oob, model_a):
    """Known answers: predicting the training samples recovers their typed alleles
    (the reference's own acceptance criterion is an accuracy threshold,
    tests/runTests.R:13-16,64-65)."""
    for model, floor in ((model_oob, 0.95), (model_a, 0.95)):
        fm = oracle.flatten(model)
        G = align_geno(model, hapmap_geno)
        a1, a2 = _truth(model, hla_type_table)
        out = oracle.predict(fm, G)
        acc = sum(oracle.compare_hla(out["h1"][i], out["h2"][i], a1[i], a2[i])
                  for i in range(model.n_samp)) / (2.0 * model.n_samp)
        assert acc >= floor
