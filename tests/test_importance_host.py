"""hlaSNPImportance on the host: the yardstick (tests/importance_reference.py) against the out-of-bag loop and
hlaCompareAllele it restates, the edge lanes of the definition, that the measure separates SNPs on the bundled models, the
per-SNP summary of the package against the yardstick's, and the Python entries' argument errors.  No GPU."""
import dataclasses
import math

import numpy as np
import pytest

import hibag_amd as hb
import importance_reference as ref
from conftest import align_geno
from hibag_amd import NA_INTEGER
from hibag_amd.importance import summarise, truth_indices
from hibag_amd.model import Classifier, HlaAttrBagObj
from test_oob_host import oracle_oob


def _hla(tab):
    return hb.HlaAlleleClass(locus="A", sample_id=list(tab["sample.id"]), allele1=list(tab["A.1"]), allele2=list(tab["A.2"]))


@pytest.fixture(scope="module")
def oob_case(oracle, model_oob, hapmap_geno, hla_type_table):
    G = align_geno(model_oob, hapmap_geno)
    return model_oob, G, ref.truth_of(model_oob, hla_type_table), ref.cached_raw("oob", oracle, model_oob, G)


@pytest.fixture(scope="module")
def a_case(oracle, model_a, hapmap_geno, hla_type_table):
    G = align_geno(model_a, hapmap_geno)
    return model_a, G, ref.truth_of(model_a, hla_type_table), ref.cached_raw("modellist_a", oracle, model_a, G)


def test_base_rows_are_the_out_of_bag_loop(oracle, oob_case):
    model, G, _, raw = oob_case
    want = oracle_oob(oracle, model, G)
    nv = raw["n_variant"]
    for k in ("h1", "h2", "prob"):
        assert np.array_equal(raw[k][nv:], want[k]), k


@pytest.mark.parametrize("thr", [float("nan"), 0.5])
def test_base_tallies_are_hlaCompareAllele(thr, oob_case, hla_type_table):
    model, _, truth, raw = oob_case
    tally = ref.knock_tally(model, raw, truth, thr)
    nv = raw["n_variant"]
    hla = _hla(hla_type_table)
    some_dropped = False
    for c, cls in enumerate(model.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        pred = hb.HlaAlleleClass(locus="A", sample_id=[model.sample_id[k] for k in oob], prob=raw["prob"][nv + c, oob],
                                 h1=raw["h1"][nv + c, oob], h2=raw["h2"][nv + c, oob], levels=model.hla_allele)
        r = hb.hlaCompareAllele(hla, pred, allele_limit=model, call_threshold=thr)
        assert (r["n.call"], r["crt.num.ind"], r["crt.num.haplo"]) == tuple(int(x) for x in tally[nv + c, 1:4]), c
        assert tally[nv + c, 4] == 0
        some_dropped = some_dropped or tally[nv + c, 1] < tally[nv + c, 0]
    if math.isfinite(thr):
        assert some_dropped                                # (the threshold does leave calls out on this model)
    # the package's truth indices are the yardstick's
    assert np.array_equal(truth_indices(model, hla), truth)


def _one_classifier(model, c):
    return dataclasses.replace(model, classifiers=[model.classifiers[c]])


def test_a_lane_that_already_misses_the_snp_equals_its_base_lane(oracle, oob_case):
    model, G, _, _ = oob_case
    m1 = _one_classifier(model, 0)
    cls = m1.classifiers[0]
    oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
    G = G.copy()
    j, lane = 2, int(oob[1])
    G[lane, int(cls.snpidx[j])] = NA_INTEGER
    raw = ref.knock_raw(oracle, m1, G)
    nv = raw["n_variant"]
    assert nv == len(cls.snpidx)
    for k in ("h1", "h2", "prob"):
        assert raw[k][j, lane] == raw[k][nv, lane], k
    assert raw["h1"][nv, lane] != NA_INTEGER
    # ... and the lanes that had the SNP typed do see the knock-out somewhere
    assert any(not np.array_equal(raw["prob"][v, oob], raw["prob"][nv, oob]) for v in range(nv))


def test_a_lane_whose_only_typed_snp_is_knocked_out_has_no_call(oracle, oob_case):
    model, G, _, _ = oob_case
    m1 = _one_classifier(model, 0)
    cls = m1.classifiers[0]
    oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
    G = G.copy()
    j, lane = 1, int(oob[0])
    keep = G[lane, int(cls.snpidx[j])]
    G[lane, :] = NA_INTEGER
    G[lane, int(cls.snpidx[j])] = keep if 0 <= keep <= 2 else 1
    raw = ref.knock_raw(oracle, m1, G)
    nv = raw["n_variant"]
    assert raw["h1"][nv, lane] != NA_INTEGER and raw["prob"][nv, lane] > 0          # the base lane: weight 1 / k
    assert raw["h1"][j, lane] == NA_INTEGER and raw["h2"][j, lane] == NA_INTEGER and raw["prob"][j, lane] == 0.0
    for v in range(nv):
        if v != j:                                          # another SNP knocked out: the lane is the base lane
            assert raw["prob"][v, lane] == raw["prob"][nv, lane]


def _discrimination(model, raw):
    nv = raw["n_variant"]
    lanes = changed = probs = 0
    for v in range(nv):
        c = int(raw["classifier"][v])
        oob = np.flatnonzero(np.asarray(model.classifiers[c].samp_num) == 0)
        lanes += len(oob)
        changed += int(np.count_nonzero((raw["h1"][v, oob] != raw["h1"][nv + c, oob]) | (raw["h2"][v, oob] != raw["h2"][nv + c, oob])))
        probs += int(np.count_nonzero(raw["prob"][v, oob] != raw["prob"][nv + c, oob]))
    return nv, lanes, changed, probs, int(len(set(int(s) for s in raw["snp"])))


def test_the_knock_out_separates_snps_on_OutOfBag_RData(oob_case):
    model, _, truth, raw = oob_case
    assert _discrimination(model, raw) == (1460, 17819, 1055, 14867, 244)
    s = ref.summary(model, ref.knock_tally(model, raw, truth))
    assert sum(1 for x in s["importance"] if x > 0) >= 50


def test_the_knock_out_separates_snps_on_ModelList_A(a_case):
    model, _, _, raw = a_case
    assert _discrimination(model, raw) == (1592, 34854, 1143, 27415, 245)


def _toy():
    """Three classifiers on five SNPs; SNP 3 has no user.  Tallies by hand: classifier 1's base row has no call at all, so
    its pairs are left out of the means; SNPs 0 and 4 tie."""
    mk = lambda idx: Classifier(snpidx=np.array(idx, np.int32), freq=np.array([1.0]), hla=np.array([0], np.int32), haplo=["0" * len(idx)])
    model = HlaAttrBagObj(n_samp=4, n_snp=5, hla_allele=["01", "02"], classifiers=[mk([0, 1]), mk([1, 2]), mk([0, 4, 2])],
                          snp_id=[f"rs{i}" for i in range(5)], snp_position=np.arange(5) * 10.0)
    tally = np.array([
        [4, 4, 1, 5, 2],     # (0, snp 0)
        [4, 4, 3, 7, 0],     # (0, snp 1)
        [4, 0, 0, 0, 4],     # (1, snp 1)
        [4, 0, 0, 0, 4],     # (1, snp 2)
        [3, 3, 1, 4, 1],     # (2, snp 0)
        [3, 2, 0, 1, 2],     # (2, snp 4)
        [3, 0, 0, 0, 3],     # (2, snp 2): nothing called after the knock-out
        [4, 4, 3, 7, 0],     # base 0
        [4, 0, 0, 0, 0],     # base 1
        [3, 3, 2, 5, 0],     # base 2
    ], np.int64)
    return model, tally


def test_summary_rules():
    model, tally = _toy()
    want = ref.summary(model, tally)
    got = summarise(model, tally, float("nan"), detail=True)
    assert list(got.n_classifier) == want["n_classifier"] == [2, 2, 2, 0, 1]
    assert list(got.n_used) == want["n_used"] == [2, 1, 0, 0, 1]
    for k in ("importance", "acc_base", "acc_drop", "importance_ind", "changed"):
        assert np.array_equal(getattr(got, k), np.array(want[k]), equal_nan=True), k
    # SNP 3 has no user, SNP 2 no usable pair: NaN; SNP 2 still has a share of changed calls
    assert math.isnan(got.importance[3]) and math.isnan(got.changed[3]) and math.isnan(got.importance[2])
    assert got.changed[2] == 1.0 and got.changed[0] == 3 / 7
    assert got.importance[0] == ((0.5 * 7 / 4 - 0.5 * 5 / 4) + (0.5 * 5 / 3 - 0.5 * 4 / 3)) / 2
    assert got.importance[1] == 0.0 and got.acc_base[1] == 0.5 * 7 / 4
    # ranking: descending, NaN last, ties in SNP order
    assert list(got.ranking()) == ref.ranking(want["importance"])
    assert list(got.ranking())[-2:] == [2, 3]
    tie = dataclasses.replace(got, importance=np.array([0.1, 0.3, np.nan, 0.1, 0.3]))
    assert list(tie.ranking()) == [1, 4, 0, 3, 2] == ref.ranking(list(tie.importance))
    assert got.snp_id == model.snp_id and np.array_equal(got.snp_position, model.snp_position)
    assert np.array_equal(got.base_tally, tally[7:]) and np.array_equal(got.variant_tally, tally[:7])
    assert list(got.variant_classifier) == [0, 0, 1, 1, 2, 2, 2] and list(got.variant_snp) == [0, 1, 1, 2, 0, 4, 2]
    assert summarise(model, tally, 0.5, detail=False).variant_tally is None


def test_argument_errors(model_oob, hapmap_geno, hla_type_table):
    hla = _hla(hla_type_table)
    with pytest.raises(TypeError, match="hlaAttrBagObj"):
        hb.hlaSNPImportance("model", hla, hapmap_geno, verbose=False)
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaSNPImportance(model_oob, hla_type_table, hapmap_geno, verbose=False)
    with pytest.raises(TypeError, match="hlaSNPGenoClass"):
        hb.hlaSNPImportance(model_oob, hla, np.zeros((3, 3)), verbose=False)
    # the cohort is matched as hlaOutOfBag matches it, with its errors -- all raised before a device is touched
    keep = [i for i, s in enumerate(hapmap_geno.sample_id) if s != model_oob.sample_id[0]]
    with pytest.raises(ValueError, match="Some of sample.id in the model do not exist in SNP genotypes."):
        hb.hlaSNPImportance(model_oob, hla, hb.hlaGenoSubset(hapmap_geno, samp_sel=keep), verbose=False)
    keep = [i for i, s in enumerate(hla.sample_id) if s != model_oob.sample_id[0]]
    with pytest.raises(ValueError, match="Some of sample.id in the model do not exist in HLA types."):
        hb.hlaSNPImportance(model_oob, hb.hlaAlleleSubset(hla, keep), hapmap_geno, verbose=False)
    keep = [i for i, s in enumerate(hapmap_geno.snp_id) if s != model_oob.snp_id[0]]
    with pytest.raises(ValueError, match="Some of snp.id in the model do not exist in SNP genotypes."):
        hb.hlaSNPImportance(model_oob, hla, hb.hlaGenoSubset(hapmap_geno, snp_sel=keep), verbose=False)
    with pytest.raises(ValueError, match="There is no sample ID in the model."):
        hb.hlaSNPImportance(dataclasses.replace(model_oob, sample_id=[]), hla, hapmap_geno, verbose=False)
    m = dataclasses.replace(model_oob, classifiers=list(model_oob.classifiers))
    m.classifiers[3] = dataclasses.replace(m.classifiers[3], samp_num=None)
    with pytest.raises(ValueError, match="There is no bootstrap sample index."):
        hb.hlaSNPImportance(m, hla, hapmap_geno, verbose=False)
    m.classifiers[3] = dataclasses.replace(model_oob.classifiers[3], samp_num=np.ones(model_oob.n_samp, np.int32))
    with pytest.raises(ValueError, match="classifier 4 has no out-of-bag sample"):
        hb.hlaSNPImportance(m, hla, hapmap_geno, verbose=False)


def test_predict_oob_knock_argument_errors(model_oob, hapmap_geno):
    """The checks of HlaAttrBagClass.predict_oob_knock come before the handle is used: a handle-less stand-in reaches them."""
    dev = object.__new__(hb.HlaAttrBagClass)
    dev.obj, dev._h = model_oob, None
    G = align_geno(model_oob, hapmap_geno)
    n, C = G.shape[0], len(model_oob.classifiers)
    sn = ref.samp_num_of(model_oob)
    with pytest.raises(ValueError, match="genomat must be"):
        dev.predict_oob_knock(G[:, :-1], sn)
    with pytest.raises(ValueError, match="samp_num must be"):
        dev.predict_oob_knock(G, sn[:-1])
    with pytest.raises(ValueError, match="samp_num must be"):
        dev.predict_oob_knock(G, sn.T)
    with pytest.raises(ValueError, match="truth must be"):
        dev.predict_oob_knock(G, sn, np.zeros((n, 3), np.int32))
    with pytest.raises(ValueError, match="truth must be"):
        dev.predict_oob_knock(G, sn, np.zeros(n, np.int32))
    with pytest.raises(TypeError, match="truth must be an integer array"):
        dev.predict_oob_knock(G, sn, np.zeros((n, 2)))
    with pytest.raises(ValueError, match="outside the model's alleles"):
        dev.predict_oob_knock(G, sn, np.full((n, 2), model_oob.n_hla, np.int32))
    with pytest.raises(ValueError, match="outside the model's alleles"):
        dev.predict_oob_knock(G, sn, np.full((n, 2), -1, np.int32))
    with pytest.raises(hb.HibagHipError, match="closed"):          # valid arguments get as far as the handle
        dev.predict_oob_knock(G, sn, np.zeros((n, 2), np.int32))
    assert C == sn.shape[0]
