"""hlaPredictFamily without a GPU: the reference of the family calls (tests/family_reference.py) reduces to the oracle's own
call, probability and dosage for founders (contract rule 9), is symmetric in father and mother (rule 10), treats a parent
without a prediction as unknown (rule 1) and skips the division for prior=None; the effect the GPU tests stand on is there
and pinned (trio weighting makes many more children's calls correct); HlaPedigree, the .fam reader, the depth sort,
hlaModelAllelePrior and hlaMendelCheck."""
import numpy as np
import pytest

from family_reference import (NA_INTEGER, conditional, correct_pairs, depths, family, family_from_postprob, founders_only,
                              model_prior)
from hibag_amd import synth
from hibag_amd.family import (HlaFamilyCalls, HlaPedigree, depth_order, hlaMendelCheck, hlaModelAllelePrior, hlaPedigreeFromFam,
                              pedigree_depth)
from hibag_amd.hibag import HlaAlleleClass
from hibag_amd.model import Classifier, HlaAttrBagObj

NA = NA_INTEGER
OUT = ("h1", "h2", "prob", "support", "dosage")


def spread_trios(n_fam=43, miss=0.85):
    """The tests' "spread" model (14 alleles, 105 cells) with n_fam trios, parents first, 85 % of the genotypes missing."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, truth, ped = synth.make_family(founders, af, n_fam, seed=12, miss=miss)
    return model, G, truth, ped


def same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# the reference's own rules on the oracle's matrix ------------------------------------------------------------------------
@pytest.mark.parametrize("vote", [1, 2])
def test_founders_are_the_oracles_own_call_and_dosage(vote, oracle):
    model, G, _, _ = spread_trios()
    G[5, :] = NA
    r = family(model, G, founders_only(len(G)), model_prior(model), vote=vote)
    for key in ("h1", "h2", "prob", "dosage"):
        assert np.array_equal(r[key], r["call"][key], equal_nan=True), (vote, key)
    assert np.array_equal(r["support"], np.cumsum(r["postprob"], axis=1)[:, -1], equal_nan=True)
    assert r["h1"][5] == NA and r["prob"][5] == 0.0 and r["support"][5] == 0.0


def test_swap_unknown_parents_and_no_prior(oracle):
    model, G, truth, ped = spread_trios()
    n, nf = model.n_hla, 43
    G[0, :] = NA                                              # the father of child 2 nf: no prediction, S = 0
    q = model_prior(model)
    r = family(model, G, ped, q)
    pp = r["postprob"]
    # parents are founders: their rows are the oracle's own, whatever their children are
    for key in ("h1", "h2", "prob", "dosage"):
        assert np.array_equal(r[key][:2 * nf], r["call"][key][:2 * nf], equal_nan=True), key
    # rule 10: father and mother swapped
    assert same(r, family_from_postprob(pp, n, ped[:, ::-1], q))
    # rule 1: a parent with every SNP missing is unknown -- the child's result is the duo's
    assert r["support"][0] == 0.0 and r["h1"][0] == NA
    duo = ped.copy()
    duo[2 * nf, 0] = -1
    assert same(r, family_from_postprob(pp, n, duo, q))
    # ... and differs from the child's own call's support: the mother still counts
    assert r["support"][2 * nf] != np.cumsum(pp[2 * nf])[-1]
    # prior=None skips the division: it equals a prior of ones bit for bit, and differs from the model's prior
    none = family_from_postprob(pp, n, ped, None)
    assert same(none, family_from_postprob(pp, n, ped, np.ones(n)))
    assert not np.array_equal(none["support"], r["support"])
    # rule 8: a three-generation chain hands the WEIGHTED (D, S) down; the grandchild is independent of unrelated samples
    chain = founders_only(len(G))
    chain[10] = (3, 4)
    chain[20] = (10, 7)
    rc = family_from_postprob(pp, n, chain, q)
    assert list(depths(chain)[[3, 10, 20]]) == [0, 1, 2]
    cut = np.array([3, 4, 7, 10, 20])
    local = np.full((5, 2), -1)
    local[3] = (0, 1)
    local[4] = (3, 2)
    rl = family_from_postprob(pp[cut], n, local, q)
    for key in OUT:
        assert np.array_equal(rc[key][cut], rl[key], equal_nan=True), key
    unweighted = founders_only(len(G))
    unweighted[20] = (10, 7)                                  # sample 10 as a founder: another result for the grandchild
    assert not same({k: rc[k][20:21] for k in OUT}, {k: family_from_postprob(pp, n, unweighted, q)[k][20:21] for k in OUT})
    # rule 7
    cond = conditional(r)
    pos = r["support"] > 0
    assert np.array_equal(cond["prob"][pos], r["prob"][pos] / r["support"][pos])


def calls_of(res, names, n):
    return HlaAlleleClass(locus="A", sample_id=list(range(n)), h1=res["h1"], h2=res["h2"], levels=names, prob=res["prob"],
                          matching=np.zeros(n), assembly="hg19", dosage=None)


def test_the_effect_is_there_and_pinned(oracle):
    """200 trios, 85 % of the genotypes missing: how many children are called with their true pair on their own, with both
    parents, with the father only; and the Mendelian-inconsistent trios before and after.  The conditions hold with wide
    room; the counts are pinned as measured on the CPU oracle."""
    model, G, truth, ped = spread_trios(200)
    q = model_prior(model)
    r = family(model, G, ped, q)
    kids = np.arange(400, 600)
    own = r["call"]
    n_own, n_trio = correct_pairs(own, truth, kids), correct_pairs(r, truth, kids)
    changed = int(np.count_nonzero((own["h1"][kids] != r["h1"][kids]) | (own["h2"][kids] != r["h2"][kids])))
    duo = ped.copy()
    duo[:, 1] = -1
    n_duo = correct_pairs(family_from_postprob(r["postprob"], model.n_hla, duo, q), truth, kids)
    names = list(model.hla_allele)
    before, after = hlaMendelCheck(calls_of(own, names, 600), ped), hlaMendelCheck(calls_of(r, names, 600), ped)
    print(f"correct child pairs: own {n_own}, trio-weighted {n_trio} ({changed} calls changed), father only {n_duo}; "
          f"inconsistent trios {before.n_inconsistent_trios} -> {after.n_inconsistent_trios} of {before.n_checked}")
    assert n_trio >= n_own + 10 and changed >= 10 and n_duo >= n_own
    assert after.n_inconsistent_trios < before.n_inconsistent_trios
    assert (n_own, n_trio, changed, n_duo) == (149, 172, 38, 151)
    assert (before.n_checked, before.n_inconsistent_trios, after.n_inconsistent_trios) == (200, 83, 54)


# HlaPedigree ---------------------------------------------------------------------------------------------------------
def test_fam_reader_and_indices(tmp_path):
    fam = tmp_path / "x.fam"
    fam.write_text("F1 dad 0 0 1 -9\nF1 mum 0 0 2 -9\nF1 kid dad mum 1 -9\n\nF2 solo 0 0 1 -9\nF2 half gone solo 2 -9\n")
    ped = hlaPedigreeFromFam(str(fam))
    assert ped.sample_id == ["dad", "mum", "kid", "solo", "half"]
    assert ped.father == [None, None, "dad", None, "gone"] and ped.mother == [None, None, "mum", None, "solo"]
    assert len(ped) == 5 and "1 with one" not in repr(ped) and "2 with two parents" in repr(ped)
    idx = ped.indices_for(["kid", "stranger", "mum", "half", "dad", "solo"])
    assert idx.dtype == np.int32 and idx.tolist() == [[4, 2], [-1, -1], [-1, -1], [-1, 5], [-1, -1], [-1, -1]]
    # parents absent from the genotypes become -1
    assert ped.indices_for(["kid", "mum"]).tolist() == [[-1, 1], [-1, -1]]
    bad = tmp_path / "bad.fam"
    bad.write_text("F1 a 0\n")
    with pytest.raises(ValueError):
        hlaPedigreeFromFam(str(bad))


def test_pedigree_rejections():
    with pytest.raises(ValueError, match="own parent"):
        HlaPedigree(["a", "b"], ["a", None], [None, None])
    with pytest.raises(ValueError, match="same person"):
        HlaPedigree(["a", "b"], [None, "a"], [None, "a"])
    with pytest.raises(ValueError, match="cycle"):
        HlaPedigree(["a", "b", "c"], ["b", "c", "a"], [None, None, None])
    with pytest.raises(ValueError, match="twice"):
        HlaPedigree(["a", "a"], [None, None], [None, None])
    with pytest.raises(ValueError, match="length"):
        HlaPedigree(["a", "b"], [None], [None, None])
    ok = HlaPedigree(["a", "b", "c"], ["0", "", "a"], [None, float("nan"), "b"])
    assert ok.father == [None, None, "a"] and ok.mother == [None, None, "b"]
    with pytest.raises(ValueError, match="cycle"):
        pedigree_depth(np.array([[1, -1], [0, -1]]))
    with pytest.raises(ValueError):
        pedigree_depth(np.array([[2, -1], [-1, -1]]))


def test_depth_sort_and_its_inverse():
    # children listed before their parents, a three-generation chain, an unrelated founder in between
    #        0: child of (3, 4)   1: founder   2: grandchild of (0, 1)   3, 4: founders   5: child of (4, -1)
    idx = np.array([[3, 4], [-1, -1], [0, 1], [-1, -1], [-1, -1], [4, -1]], np.int32)
    order, inverse, sorted_idx, depth = depth_order(idx)
    assert depth.tolist() == [1, 0, 2, 0, 0, 1]
    assert order.tolist() == [1, 3, 4, 0, 5, 2]               # stable within a depth
    assert np.array_equal(inverse[order], np.arange(6)) and np.array_equal(order[inverse], np.arange(6))
    assert sorted_idx.tolist() == [[-1, -1], [-1, -1], [-1, -1], [1, 2], [2, -1], [3, 0]]
    assert np.array_equal(depths(sorted_idx), depth[order])   # parents precede their children now
    # the sorted pedigree names the same people
    back = np.where(sorted_idx >= 0, order[np.maximum(sorted_idx, 0)], -1)
    assert np.array_equal(back[inverse], idx)
    # a pedigree that is already parents-first is left alone, depth-sorted or not
    fine = np.array([[-1, -1], [-1, -1], [0, 1], [-1, -1], [2, 3]], np.int32)
    order, inverse, sorted_idx, depth = depth_order(fine)
    assert order.tolist() == [0, 1, 2, 3, 4] and sorted_idx is not None and np.array_equal(sorted_idx, fine)
    assert depth.tolist() == [0, 0, 1, 0, 2]
    e = depth_order(np.zeros((0, 2), np.int32))
    assert len(e[0]) == 0 and e[2].shape == (0, 2)


def test_model_allele_prior_on_a_model_written_out_by_hand():
    c1 = Classifier([0, 1], [0.5, 0.25, 0.25], [0, 0, 2], ["00", "01", "11"])
    c2 = Classifier([1, 2], [0.125, 0.875], [0, 1], ["00", "11"])
    model = HlaAttrBagObj(0, 3, ["a", "b", "c", "d"], [c1, c2])
    q = hlaModelAllelePrior(model)
    # allele a: (0.75 + 0.125) / 2, b: (0 + 0.875) / 2, c: (0.25 + 0) / 2, d: in no classifier -> 1.0
    assert q.tolist() == [0.4375, 0.4375, 0.125, 1.0]
    assert np.array_equal(q, model_prior(model))
    big, _, _ = synth.make_model("hla-a-small", seed=11)
    assert np.array_equal(hlaModelAllelePrior(big), model_prior(big))
    assert not np.allclose(hlaModelAllelePrior(big), big.hla_freq)      # (the object's hla_freq is another thing)


def test_mendel_check_and_family_calls():
    names = ["a", "b", "c"]
    # 0 father (a, b), 1 mother (b, c), 2 child (a, c) ok, 3 child (a, a) not, 4 duo child of 1 (a, b) ok, 5 duo child of 1
    # (a, a) not, 6 child of an uncalled parent only: not checked, 7 uncalled child
    h1 = np.array([0, 1, 0, 0, 0, 0, 0, NA], np.int32)
    h2 = np.array([1, 2, 2, 0, 1, 0, 0, NA], np.int32)
    ped = np.array([[-1, -1], [-1, -1], [0, 1], [0, 1], [-1, 1], [1, -1], [7, -1], [0, 1]], np.int32)
    hla = HlaAlleleClass(locus="A", sample_id=[f"s{i}" for i in range(8)], h1=h1, h2=h2, levels=names, prob=np.ones(8),
                         matching=np.ones(8), assembly="hg19", dosage=None)
    m = hlaMendelCheck(hla, ped)
    assert m.child.tolist() == [2, 3, 4, 5] and m.consistent.tolist() == [True, False, True, False]
    assert m.n_parents.tolist() == [2, 2, 1, 1] and (m.n_checked, m.n_inconsistent, m.n_inconsistent_trios) == (4, 2, 1)
    byid = HlaPedigree([f"s{i}" for i in (2, 3)], ["s0", "s0"], ["s1", "s1"])
    assert hlaMendelCheck(hla, byid).n_inconsistent_trios == 1
    # HlaFamilyCalls holds the conditional values (rule 7) next to the joint ones
    sup = np.array([0.5, 0.0, 2.0])
    r = HlaFamilyCalls("A", ["x", "y", "z"], names, h1[:3], h2[:3], np.array([0.25, 0.0, 0.5]), sup, np.ones(3),
                       np.array([[0.5, 0.25, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 2.0]]), ped[:3], np.array([0, 0, 1]))
    assert r.prob.tolist() == [0.5, 0.0, 0.25] and r.dosage.shape == (3, 3)
    assert r.dosage.T.tolist() == [[1.0, 0.5, 0.5], [0.0, 0.0, 0.0], [0.5, 0.5, 1.0]]
    assert r.calls().allele1 == ["a", "b", "a"] and hlaMendelCheck(r, ped[:3]).n_checked == 1
