"""hlaPredictTopK on the GPU: hibag_hip_predict_topk and its routes equal, every sample, every rank and both vote methods,
to the reference selection (tests/topk_reference.py: a stable descending sort of the CPU oracle's posterior matrix, values
> 0 only); rank 0 bit for bit the library's own call; the model's other outputs untouched; invalid arguments rejected.
Every comparison is exact equality (NaN == NaN for probabilities): there is no tolerance in this feature."""
import ctypes as C
import os

import numpy as np
import pytest

import hibag_amd as hb
from conftest import REFDATA, align_geno
from hibag_amd import NA_INTEGER, _lib, synth
from hibag_amd._lib import TOPK_MAX
from oracle_full import cohort
from topk_reference import assert_topk_equal, select, topk

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def check_ranks(got, raw, what=""):
    """Case 9: rank 0, prob[:, 0] and matching are predict_raw's h1, h2, prob, matching bit for bit; every row's prob is
    non-increasing over the listed ranks; ranks are filled from the front."""
    assert np.array_equal(got["h1"][:, 0], raw["h1"]) and np.array_equal(got["h2"][:, 0], raw["h2"]), what
    assert np.array_equal(got["prob"][:, 0], raw["prob"], equal_nan=True), what
    assert np.array_equal(got["matching"], raw["matching"], equal_nan=True), what
    listed = got["h1"] != NA
    assert np.array_equal(listed, got["h2"] != NA) and np.all(listed[:, :-1] >= listed[:, 1:]), what
    p = got["prob"]
    both = listed[:, :-1] & listed[:, 1:]
    assert np.all(p[:, :-1][both] >= p[:, 1:][both]) and np.all(p[listed] > 0), what
    assert np.all((p[~listed] == 0) | np.isnan(p[~listed])), what


def run_case(model, G, k, votes=(1, 2), what=""):
    """predict_topk against the reference, both votes; returns {vote: (got, want)}."""
    out = {}
    dev = hb.hlaModelFromObj(model)
    try:
        for vote in votes:
            got = dev.predict_topk(G, k, vote)
            raw = dev.predict_raw(G, vote, want_dosage=False)
            assert dev.status() == 0 and dev.handover_faults() == 0
            want = topk(model, G, k, vote=vote)
            assert got["h1"].shape == (len(G), k) and got["h1"].dtype == np.int32 and got["prob"].dtype == np.float64
            assert_topk_equal(got, want, f"{what} k={k} vote={vote}")
            check_ranks(got, raw, f"{what} k={k} vote={vote}")
            out[vote] = (got, want)
    finally:
        dev.close()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, TOPK_MAX])
@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_fixture_models_on_the_hapmap_genotypes(which, k, request, hapmap_geno):
    model = request.getfixturevalue(which)
    G = align_geno(model, hapmap_geno, hapmap_geno.sample_id)
    run_case(model, G, k, what=which)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_hla_b_shape_100_classifiers_2048_samples():
    """oracle_full's "structured" recipe: groups that miss every SNP of some classifiers, an all-NA last sample."""
    model, G, _ = cohort("hla-b", 2048, recipe="structured")
    for vote, (got, _) in run_case(model, G, 4, what="hla-b").items():
        assert np.all(got["h1"][-1] == NA) and np.all(got["h2"][-1] == NA) and np.isnan(got["matching"][-1]), vote


# 3 ---------------------------------------------------------------------------------------------------------------
def wide_case():
    """One-step FP4, int8, multi-step FP4 and VALU (> 112 SNPs) classifiers; 300 samples (not a multiple of 64: a partial
    group of 44), one with every SNP missing, some that miss all SNPs of a classifier."""
    counts = [12, 113, 18, 40, 24, 30, 31, 32, 56, 84, 100, 120, 128, 20]
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(counts), snp_counts=counts)
    G, _ = synth.make_samples(founders, af, 300, seed=8)
    G[0, :] = NA
    G[np.ix_(range(64, 80), model.classifiers[0].snpidx)] = NA
    G[np.ix_(range(70, 90), model.classifiers[3].snpidx[1:])] = NA
    return model, G


def test_wide_classifiers_and_a_partial_group():
    model, G = wide_case()
    run_case(model, G, 4, what="wide")
    run_case(model, G, 11, votes=(1,), what="wide")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_drb1_shape_and_the_models_own_prediction_is_untouched():
    """The large-n_cell, store-every-cell layout (pass 2 = k_accum_cells)."""
    model, founders, af = synth.make_model("hla-drb1", n_classifier=8)
    G, _ = synth.make_samples(founders, af, 200)
    G[7, :] = NA
    dev = hb.hlaModelFromObj(model)
    try:
        assert dev.stored_cells() > 0 and dev.second_pass_pairs() == 0
        before = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        for k in (4, 7, TOPK_MAX):
            for vote in (1, 2):
                got = dev.predict_topk(G, k, vote)
                assert_topk_equal(got, topk(model, G, k, vote=vote), f"drb1 k={k} vote={vote}")
                check_ranks(got, dev.predict_raw(G, vote, want_dosage=False), f"drb1 k={k} vote={vote}")
        after = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        assert dev.status() == 0
    finally:
        dev.close()
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key


# 5 ---------------------------------------------------------------------------------------------------------------
def two_allele_case():
    c1 = hb.Classifier([0, 1, 2, 3], [0.3, 0.3, 0.4], [0, 1, 1], ["0000", "0101", "1111"])
    c2 = hb.Classifier([1, 4], [0.5, 0.5], [0, 1], ["00", "11"])
    model = hb.HlaAttrBagObj(0, 5, ["a", "b"], [c1, c2])
    G = np.array([[0, 0, 0, 0, 0], [2, 2, 2, 2, 2], [0, 1, 0, 1, 1], [1, 1, 1, 1, 1], [NA] * 5, [0, NA, 2, 1, NA]], np.int32)
    return model, G


def test_two_alleles_more_ranks_than_cells():
    model, G = two_allele_case()
    for vote, (got, want) in run_case(model, G, TOPK_MAX, what="2 alleles").items():
        assert model.n_cell == 3 and ((want["postprob"] > 0).sum(axis=1) < TOPK_MAX).all()       # the corner is there
        assert np.all(got["h1"][:, 3:] == NA) and np.all(got["h2"][:, 3:] == NA) and np.all(got["prob"][:, 3:] == 0.0)
        assert (got["h1"][:, 0] != NA).any()


# 6 ---------------------------------------------------------------------------------------------------------------
def mirrored_case():
    """Two alleles with the SAME haplotypes and frequencies make bit-equal cell sums, and samples built from one haplotype
    of the mirrored pair and one of a third allele put the tie at the top: cells (0, 2) and (1, 2)."""
    rng = np.random.default_rng(77)
    n_snp, k = 40, 18
    cls, pats_all = [], []
    for j in range(6):
        idx = np.sort(rng.choice(n_snp, k, replace=False))
        a = ["".join(rng.choice(["0", "1"], k)) for _ in range(3)]
        cpat = ["".join(rng.choice(["0", "1"], k)) for _ in range(2)]
        fa = rng.uniform(0.05, 0.3, 3)
        fc = rng.uniform(0.05, 0.3, 2)
        cls.append(hb.Classifier(snpidx=idx, freq=np.concatenate([fa, fa, fc]), hla=np.array([0] * 3 + [1] * 3 + [2] * 2, np.int32),
                                 haplo=a + a + cpat))                                   # allele 0, its mirror allele 1, allele 2
        pats_all.append((idx, a, cpat))
    model = hb.HlaAttrBagObj(n_samp=0, n_snp=n_snp, hla_allele=["a", "a'", "c"], classifiers=cls)
    rows = []
    for t in range(96):
        idx, a, cpat = pats_all[t % 6]
        g = rng.choice(np.array([0, 1, 2], np.int32), n_snp)
        g[idx] = np.array([int(x) + int(y) for x, y in zip(a[t % 3], cpat[t % 2])], np.int32)
        if t % 7 == 0:
            g[rng.choice(n_snp, 3, replace=False)] = NA
        rows.append(g)
    return model, np.stack(rows).astype(np.int32)


def test_tied_cells_come_in_adjacent_ranks_in_cell_order():
    model, G = mirrored_case()
    for vote, (got, want) in run_case(model, G, 4, what="mirrored").items():
        tied = (want["prob"][:, 0] == want["prob"][:, 1]) & (want["h1"][:, 1] != NA)
        assert tied.any(), vote                                                     # the corner is there
        # cell order: (0, 2) is cell 2, (1, 2) is cell 4 -- the earlier twin first, the probabilities bit-equal
        top2 = tied & (got["h1"][:, 0] == 0) & (got["h2"][:, 0] == 2) & (got["h1"][:, 1] == 1) & (got["h2"][:, 1] == 2)
        assert top2.any() or vote == 2, vote      # (the majority vote gives the later twin no votes: its ties are other cells)
        assert np.array_equal(got["prob"][tied, 0].view(np.uint64), got["prob"][tied, 1].view(np.uint64))
        cell = lambda h1, h2: h2 + h1 * (2 * 3 - h1 - 1) // 2
        assert np.all(cell(got["h1"][tied, 0], got["h2"][tied, 0]) < cell(got["h1"][tied, 1], got["h2"][tied, 1]))


# 7 ---------------------------------------------------------------------------------------------------------------
def underflow_case():
    """A classifier whose every pair is >= 65 mismatches away has total 0, so 1/total = inf and 0 * inf = NaN poisons the
    whole sample (src/LibHLA.cpp:1826-1828)."""
    k = 100
    far = hb.Classifier(np.arange(k), [0.5, 0.5], [0, 1], ["1" * k, "1" * k])
    near = hb.Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    model = hb.HlaAttrBagObj(0, k, ["a", "b", "c"], [near, far])
    G = np.zeros((3, k), np.int32)        # all homozygous B: 2 mismatches per SNP against "111..."
    G[1, 40:] = NA                        # 40 typed SNPs -> 80 mismatches: exact zero; sample 2 sees neither
    G[2, :] = NA
    return model, G


def test_nan_posteriors_give_na_ranks():
    model, G = underflow_case()
    res = run_case(model, G, 3, what="underflow")
    got, want = res[1]
    assert np.isnan(want["postprob"][0]).all() and want["call"]["h1"][0] == NA           # the corner is there
    assert np.all(got["h1"][0] == NA) and np.all(got["h2"][0] == NA)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_cohort_larger_than_a_batch_host_entry_and_device_entry():
    """More samples than batch_limit(): the host entry goes through the three-stream slices, the device entry through
    several batches of one resident matrix; both compared in full."""
    import torch
    model, founders, af = synth.make_model("hla-a-small")
    dev = hb.hlaModelFromObj(model)
    try:
        n = dev.batch_limit() + 3000 + 17
        G, _ = synth.make_samples(founders, af, n, seed=31)
        G[n - 1, :] = NA
        k = 4
        want = topk(model, G, k)
        got = dev.predict_topk(G, k, 1)
        assert dev.status() == 0 and dev.handover_faults() == 0
        assert_topk_equal(got, want, "host entry")
        check_ranks(got, dev.predict_raw(G, 1, want_dosage=False), "host entry")
        tdev = torch.device("cuda", dev.device())
        dg = torch.from_numpy(G).to(tdev)
        o = dict(h1=torch.empty((n, k), dtype=torch.int32, device=tdev), h2=torch.empty((n, k), dtype=torch.int32, device=tdev),
                 prob=torch.empty((n, k), dtype=torch.float64, device=tdev), matching=torch.empty(n, dtype=torch.float64, device=tdev))
        torch.cuda.synchronize(tdev)
        st = torch.cuda.current_stream(tdev)
        dev.predict_topk_device(dg.data_ptr(), n, k, o["h1"].data_ptr(), o["h2"].data_ptr(), o["prob"].data_ptr(),
                                o["matching"].data_ptr(), vote_method=1, stream=st.cuda_stream)
        st.synchronize()
        assert dev.status() == 0
        for key in ("h1", "h2", "prob", "matching"):
            assert np.array_equal(o[key].cpu().numpy(), got[key], equal_nan=True), key
    finally:
        dev.close()


@pytest.mark.parametrize("which_pass", [1, 2])
def test_host_entry_repairs_a_dropped_handover(which_pass):
    """The benchmark batch (both passes have cut tails): with the first hand-over of a pass dropped the poisoned lists are
    never returned -- the library runs the call again without hand-overs."""
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 10_000)
    m = hb.hlaModelFromObj(model)
    try:
        m.inject_handover_fault(which_pass)
        got = m.predict_topk(G, 4, 1)
        assert m.handover_faults() == 1 and m.status() == 0
    finally:
        m.close()
    assert not np.isnan(got["prob"]).any()
    assert_topk_equal(got, topk(model, G, 4), f"repair, pass {which_pass}")


# 10 --------------------------------------------------------------------------------------------------------------
def _select_from(res, k, n_hla):
    """The reference selection applied to hlaPredict(type="response+prob")'s matrix [n_cell, n_samp]."""
    return select(np.ascontiguousarray(res.postprob.T), k, n_hla)


def _assert_top_is(top, res, k, n_hla, what):
    want = _select_from(res, k, n_hla)
    want["matching"] = res.matching
    assert_topk_equal({"h1": top.h1, "h2": top.h2, "prob": top.prob, "matching": top.matching}, want, what)
    assert top.sample_id == list(res.sample_id) and top.assembly == res.assembly and top.k == k
    assert np.array_equal(top.n_listed, (want["h1"] != NA).sum(axis=1))


def _assert_best_is(best, resp, what):
    assert np.array_equal(best.h1, resp.h1) and np.array_equal(best.h2, resp.h2), what
    assert np.array_equal(best.prob, resp.prob, equal_nan=True) and np.array_equal(best.matching, resp.matching, equal_nan=True), what
    assert best.allele1 == resp.allele1 and best.allele2 == resp.allele2 and best.sample_id == resp.sample_id, what
    assert best.locus == resp.locus and best.assembly == resp.assembly, what


def mapped_cohort(model, G):
    """An hlaSNPGenoClass whose SNPs are a reordered subset of the model's, a third of them with reversed alleles, plus
    SNPs the model does not know (the recipe of tests/test_hip_bed.py's mapped test)."""
    S, n_samp = model.n_snp, len(G)
    rng = np.random.default_rng(13)
    keep = rng.random(S) < 0.9
    flip = rng.random(S) < 0.33
    extra = 17
    order = rng.permutation(int(keep.sum()) + extra)
    rows, ids, pos, alle = [], [], [], []
    for j in np.where(keep)[0]:
        g = G[:, j].copy()
        if flip[j]:
            g = np.where(g == NA, NA, 2 - g)
        rows.append(g); ids.append(model.snp_id[j]); pos.append(model.snp_position[j])
        alle.append("G/A" if flip[j] else "A/G")
    for e in range(extra):
        rows.append(rng.integers(0, 3, n_samp).astype(np.int32)); ids.append(f"x{e}"); pos.append(1000 + e); alle.append("C/T")
    assert (flip & keep).any() and not keep.all()
    return hb.HlaSNPGeno(genotype=np.array([rows[i] for i in order], np.int32), sample_id=[f"s{i}" for i in range(n_samp)],
                         snp_id=[ids[i] for i in order], snp_position=np.array([pos[i] for i in order], np.float64),
                         snp_allele=[alle[i] for i in order], assembly="hg19")


@pytest.mark.parametrize("vote", ["prob", "majority"])
def test_hla_predict_topk_end_to_end(vote, model_a, hapmap_geno):
    k = 3
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 333, seed=12)
    G[5, :] = NA
    m = hb.hlaModelFromObj(model)
    try:
        # the mapped route: both memory orders of the cohort's own matrix
        snp = mapped_cohort(model, G)
        for order in ("C", "F"):
            snp.genotype = np.asarray(snp.genotype, order=order)
            with pytest.warns(UserWarning, match="No prediction output"):
                top = hb.hlaPredictTopK(m, snp, k=k, vote=vote, verbose=False)
            with pytest.warns(UserWarning):
                res = hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False)
                resp = hb.hlaPredict(m, snp, type="response", vote=vote, verbose=False)
            _assert_top_is(top, res, k, model.n_hla, f"HlaSNPGeno {order}")
            _assert_best_is(top.best(), resp, f"HlaSNPGeno {order}")
            assert top.allele1[0] == resp.allele1 and top.allele2[1] == top.rank(1).allele2 and top.levels == model.hla_allele
        # a numeric matrix [n.snp, n.samp] in C order and in Fortran order, and a vector
        for mat, what in ((np.ascontiguousarray(G[:100].T), "C"), (np.asfortranarray(G[:100].T), "F"),
                          (np.ascontiguousarray(G[:100].T).astype(np.float64), "float"), (G[3].copy(), "vector")):
            top = hb.hlaPredictTopK(m, mat, k=k, vote=vote, verbose=False)
            res = hb.hlaPredict(m, mat, type="response+prob", vote=vote, verbose=False)
            _assert_top_is(top, res, k, model.n_hla, what)
            _assert_best_is(top.best(), hb.hlaPredict(m, mat, type="response", vote=vote, verbose=False), what)
    finally:
        m.close()
    # the lazily opened BED file of the HapMap fixture
    lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
    m = hb.hlaModelFromObj(model_a)
    try:
        top = hb.hlaPredictTopK(m, lazy, k=TOPK_MAX, vote=vote, match_type="RefSNP", verbose=False)
        res = hb.hlaPredict(m, lazy, type="response+prob", vote=vote, match_type="RefSNP", verbose=False)
        _assert_top_is(top, res, TOPK_MAX, model_a.n_hla, "BED")
        _assert_best_is(top.best(), hb.hlaPredict(m, lazy, type="response", vote=vote, match_type="RefSNP", verbose=False), "BED")
        assert np.all(top.coverage[top.n_listed > 0] > 0) and np.all(top.coverage[top.n_listed == 0] == 0)
    finally:
        m.close()


def test_verbose_text(model_a, hapmap_geno, capsys):
    m = hb.hlaModelFromObj(model_a)
    try:
        hb.hlaPredictTopK(m, hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(5))), k=2, match_type="RefSNP")
    finally:
        m.close()
    text = capsys.readouterr().out
    assert "the 2 best allele pairs per sample" in text and "# of samples: 5" in text


# 11 --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_call(model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    n, k = len(G), 3
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    h1, h2 = np.empty((n, TOPK_MAX + 1), np.int32), np.empty((n, TOPK_MAX + 1), np.int32)
    pr, mt = np.empty((n, TOPK_MAX + 1)), np.empty(n)
    dev = hb.hlaModelFromObj(model_a)
    try:
        call = lambda kk, a, b, c, d, n_samp=n, vote=1: L.hibag_hip_predict_topk(dev.handle, p(G), n_samp, vote, kk, p(a), p(b), p(c), p(d))
        for bad_k in (0, TOPK_MAX + 1, -3):
            assert call(bad_k, h1, h2, pr, mt) == -1 and str(TOPK_MAX) in L.hibag_hip_last_error().decode()
        for args in ((None, h2, pr, mt), (h1, None, pr, mt), (h1, h2, None, mt)):
            assert call(k, *args) == -1 and "required" in L.hibag_hip_last_error().decode()
        assert call(k, h1, h2, pr, mt, n_samp=-1) == -1
        assert call(k, h1, h2, pr, mt, vote=3) == -1 and "vote_method" in L.hibag_hip_last_error().decode()
        col = np.arange(model_a.n_snp, dtype=np.int32)
        assert L.hibag_hip_predict_topk_mapped(dev.handle, p(G), n, G.shape[1], p(col), None, 1, 0, p(h1), p(h2), p(pr), p(mt)) == -1
        assert L.hibag_hip_predict_topk_snp_major(dev.handle, p(G), n, n, G.shape[1], None, None, 1, TOPK_MAX + 1, p(h1), p(h2), p(pr), p(mt)) == -1
        assert L.hibag_hip_predict_topk_bed(dev.handle, BED.encode(), 90, 5316, p(col), None, 1, 0, p(h1), p(h2), p(pr), p(mt)) == -1
        assert L.hibag_hip_predict_topk_device(dev.handle, p(G), n, 1, 0, p(h1), p(h2), p(pr), p(mt), None) == -1
        assert dev.status() == 0
        # the model is still usable, and matching may be NULL
        a = np.empty((n, k), np.int32); b = np.empty((n, k), np.int32); c = np.empty((n, k))
        assert call(k, a, b, c, None) == 0
        got = dev.predict_topk(G, k, 1)
        assert np.array_equal(a, got["h1"]) and np.array_equal(b, got["h2"]) and np.array_equal(c, got["prob"], equal_nan=True)
        assert_topk_equal(got, topk(model_a, G, k), "after the rejected calls")
        assert call(k, None, None, None, None, n_samp=0) == 0                          # nothing to write
    finally:
        dev.close()
