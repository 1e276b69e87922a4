"""hlaPredictTopK on the host: the reference selection (tests/topk_reference.py) on hand-made columns -- ties in cell order,
zeros and NaN never listed, padding -- and against the oracle's own call on the HapMap fixture; the two forms of the
selection agree; and the parts of the feature that need no device: the exported names, the declared symbols, the checks
of `k`, the result object assembled from given arrays."""
import os
import re

import numpy as np
import pytest

import hibag_amd as hb
from conftest import ROOT, align_geno
from hibag_amd import NA_INTEGER
from topk_reference import pair_of_cell, select, select_fast, topk

NA = NA_INTEGER
NAN = float("nan")


def _cells(n_hla):
    """(h1, h2) of every cell in cell order, by the loop nest itself."""
    return [(i, j) for i in range(n_hla) for j in range(i, n_hla)]


@pytest.mark.parametrize("n_hla", [1, 2, 3, 7, 50])
def test_cell_to_pair_is_the_loop_nest(n_hla):
    want = np.array(_cells(n_hla), np.int32)
    h1, h2 = pair_of_cell(np.arange(len(want)), n_hla)
    assert np.array_equal(h1, want[:, 0]) and np.array_equal(h2, want[:, 1])
    h1, h2 = pair_of_cell(np.array([-1, 0]), n_hla)
    assert (h1[0], h2[0]) == (NA, NA) and (h1[1], h2[1]) == (0, 0)


def test_ties_come_out_in_cell_order():
    #                cell: 0    1    2    3    4    5      (3 alleles: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2))
    pp = np.array([[0.1, 0.3, 0.1, 0.3, 0.1, 0.1],
                   [0.25, 0.25, 0.25, 0.25, 0.0, 0.0]])
    for f in (select, select_fast):
        r = f(pp, 4, 3)
        assert r["h1"].dtype == np.int32 and r["prob"].shape == (2, 4)
        assert r["h1"].tolist() == [[0, 1, 0, 0], [0, 0, 0, 1]] and r["h2"].tolist() == [[1, 1, 0, 2], [0, 1, 2, 1]]
        assert r["prob"].tolist() == [[0.3, 0.3, 0.1, 0.1], [0.25, 0.25, 0.25, 0.25]]


def test_zeros_and_nan_are_never_listed_and_short_lists_are_padded():
    pp = np.array([[0.0, 0.7, NAN, 0.0, 0.3, -0.0],
                   [NAN] * 6,
                   [0.0] * 6,
                   [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    for f in (select, select_fast):
        r = f(pp, 3, 3)
        assert r["h1"].tolist() == [[0, 1, NA], [NA] * 3, [NA] * 3, [0, NA, NA]]
        assert r["h2"].tolist() == [[1, 2, NA], [NA] * 3, [NA] * 3, [0, NA, NA]]
        assert r["prob"].tolist() == [[0.7, 0.3, 0.0], [0.0] * 3, [0.0] * 3, [1.0, 0.0, 0.0]]
    # more ranks than cells
    r = select(pp[:1], 8, 3)
    assert r["h1"].shape == (1, 8) and r["h1"][0, 2:].tolist() == [NA] * 6 and r["prob"][0].tolist() == [0.7, 0.3] + [0.0] * 6
    assert select_fast(pp[:1], 8, 3)["h2"].tolist() == r["h2"].tolist()


@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_the_two_forms_agree(k):
    """Random matrices made of few distinct values: ties everywhere, also across the partition's cut; zeros and NaN."""
    rng = np.random.default_rng(5 + k)
    n_hla = 9
    P = n_hla * (n_hla + 1) // 2
    pp = rng.choice(np.array([0.0, 0.0, 0.01, 0.02, 0.05, 0.2, NAN]), size=(400, P))
    pp[:50] = rng.random((50, P))
    pp[50:60, 1:] = 0.0                                        # fewer than k positive cells
    a, b = select(pp, k, n_hla), select_fast(pp, k, n_hla)
    for key in ("h1", "h2", "prob"):
        assert np.array_equal(a[key], b[key]), key
    listed = a["h1"] != NA
    assert np.all(np.diff(np.where(listed, a["prob"], -1.0), axis=1) <= 0)                   # non-increasing, NA ranks last
    assert (listed.sum(axis=1) < k).any() or k == 1


def test_rank_0_is_the_oracles_own_call(model_a, hapmap_geno, oracle):
    G = align_geno(model_a, hapmap_geno, hapmap_geno.sample_id)
    for vote in (1, 2):
        r = topk(model_a, G, 3, vote=vote)
        assert np.array_equal(r["h1"][:, 0], r["call"]["h1"]) and np.array_equal(r["h2"][:, 0], r["call"]["h2"])
        assert np.array_equal(r["prob"][:, 0], r["call"]["prob"], equal_nan=True)
        assert (r["h1"][:, 0] != NA).any()
        again = select_fast(r["postprob"], 3, model_a.n_hla)
        for key in ("h1", "h2", "prob"):
            assert np.array_equal(r[key], again[key]), key


def test_names_are_exported():
    assert "hlaPredictTopK" in hb.__all__ and "HlaTopCalls" in hb.__all__
    assert callable(hb.hlaPredictTopK) and isinstance(hb.HlaTopCalls, type)
    assert hasattr(hb.HlaAttrBagClass, "predict_topk")


TOPK_ENTRIES = ["hibag_hip_predict_topk", "hibag_hip_predict_topk_device", "hibag_hip_predict_topk_mapped",
                "hibag_hip_predict_topk_snp_major", "hibag_hip_predict_topk_bed"]


def test_symbols_are_declared_and_exported():
    from hibag_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    declared = set(re.findall(r"\b(hibag_hip_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in TOPK_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    m = re.search(r"#define\s+HIBAG_HIP_TOPK_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.TOPK_MAX and _lib.TOPK_MAX >= 8
    assert re.search(r"#define\s+HIBAG_HIP_ABI_VERSION\s+7\b", hdr) and "within version 7" in hdr
    # one more argument (k) than the sibling entry has outputs to drop (H1, H2, max_prob, dosage, postprob -> h1, h2, prob)
    assert len(L.hibag_hip_predict_topk.argtypes) == len(L.hibag_hip_predict.argtypes) - 1
    assert len(L.hibag_hip_predict_topk_bed.argtypes) == len(L.hibag_hip_predict_bed.argtypes) - 1


def _shell(obj):
    """An hlaAttrBagClass without a device model: enough for the checks that come before any device work."""
    m = object.__new__(hb.HlaAttrBagClass)
    m.obj, m._h = obj, None
    return m


def test_k_is_checked_before_any_device_work(model_a):
    from hibag_amd import _lib
    from hibag_amd.hibag import topk_k
    assert topk_k(1) == 1 and topk_k(np.int32(_lib.TOPK_MAX)) == _lib.TOPK_MAX and topk_k(4.0) == 4
    G = np.zeros((model_a.n_snp, 3), np.int32)
    m = _shell(model_a)
    for bad in (0, _lib.TOPK_MAX + 1, -1, 2.5, "3", None, True):
        with pytest.raises(ValueError, match=str(_lib.TOPK_MAX)):
            topk_k(bad)
        with pytest.raises(ValueError, match=str(_lib.TOPK_MAX)):
            hb.hlaPredictTopK(m, G, k=bad, verbose=False)
        with pytest.raises(ValueError, match=str(_lib.TOPK_MAX)):
            m.predict_topk(G.T, bad)
    with pytest.raises(TypeError):
        hb.hlaPredictTopK(model_a, G, verbose=False)              # an hlaAttrBagObj is not a device model
    with pytest.raises(ValueError):
        hb.hlaPredictTopK(m, G, vote="mean", verbose=False)
    with pytest.raises(TypeError):
        hb.hlaPredictTopK(m, G, cl=[0], verbose=False)            # several devices: not part of this function
    with pytest.raises(TypeError):
        hb.hlaPredictTopK(m, np.array([["a"] * 3] * model_a.n_snp), verbose=False)
    with pytest.raises(ValueError):
        hb.hlaPredictTopK(m, G[:-1], verbose=False)


def test_the_result_object(model_a):
    al = model_a.hla_allele
    h1 = np.array([[0, 1, NA], [2, NA, NA], [NA, NA, NA]], np.int32)
    h2 = np.array([[1, 1, NA], [3, NA, NA], [NA, NA, NA]], np.int32)
    prob = np.array([[0.6, 0.3, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    mt = np.array([0.5, 0.25, NAN])
    ids = ["a", "b", "c"]
    top = hb.HlaTopCalls(model_a.hla_locus, ids, 3, h1, h2, prob, mt, assembly="hg19", levels=al)
    assert top.k == 3 and top.locus == model_a.hla_locus and top.sample_id == ids and top.assembly == "hg19"
    assert np.array_equal(top.n_listed, [2, 1, 0]) and np.array_equal(top.coverage, prob.sum(axis=1))
    assert top.allele1 == [[al[0], al[2], None], [al[1], None, None], [None] * 3]
    assert top.allele2 == [[al[1], al[3], None], [al[1], None, None], [None] * 3]
    b = top.best()
    assert isinstance(b, hb.HlaAlleleClass) and np.array_equal(b.h1, h1[:, 0]) and np.array_equal(b.h2, h2[:, 0])
    assert np.array_equal(b.prob, prob[:, 0]) and b.matching is mt and b.sample_id == ids and b.assembly == "hg19"
    assert b.allele1 == [al[0], al[2], None] and b.dosage is None and b.postprob is None
    r1 = top.rank(1)
    assert r1.allele1 == [al[1], None, None] and np.array_equal(r1.prob, [0.3, 0.0, 0.0])
    true = hb.HlaAlleleClass(locus=model_a.hla_locus, sample_id=ids, allele1=[al[1], al[0], al[0]], allele2=[al[1], al[0], al[0]])
    assert hb.hlaCompareAllele(true, r1)["total.num.ind"] == 1
    for bad in (3, -1, 1.0):
        with pytest.raises(IndexError):
            top.rank(bad)
    with pytest.raises(ValueError):
        hb.HlaTopCalls(model_a.hla_locus, ids, 2, h1, h2, prob, mt, levels=al)
