"""A per-sample classifier mask on the GPU: hibag_hip_predict_masked bit-identical, in all six outputs, to the oracle's
prediction of every sample's own sub-model (tests/masked_reference.py), and hlaOutOfBagEnsemble equal to hlaCompareAllele
applied to that yardstick."""
import ctypes as C
import dataclasses
import warnings

import numpy as np
import pytest

import hibag_amd as hb
import masked_reference as MR
from conftest import align_geno
from hibag_amd import NA_INTEGER, _lib, synth

pytestmark = pytest.mark.gpu

VOTES = (1, 2)


def _masked(dev, G, use, vote):
    return dev.predict_masked(G, use, vote_method=vote, want_dosage=True, want_prob=True)


def _samp_num(model):
    return np.stack([np.asarray(c.samp_num, np.int32) for c in model.classifiers])


# ---- 1. engine mix, batch boundaries, crafted columns ---------------------------------------------------------------

ALL_ONES, ALL_ZEROS, ONLY_0, ONLY_9 = (10, 140, 290), (11, 130, 299), (12, 200), (13, 260)


@pytest.fixture(scope="module")
def mix_case():
    """tests/test_hip_oob.py's synth_case recipe (one-step FP4, multi-step FP4 and VALU classifiers, a seeded bootstrap,
    samples that miss some and all of a classifier's SNPs) with the bootstrap's out-of-bag mask and crafted columns in each
    of the three batches HIBAG_MASK_BATCH=128 makes of the 300 samples; the yardstick of both votes, computed once."""
    counts = [12, 18, 24, 30, 31, 40, 56, 84, 100, 113, 120, 128]
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(counts), snp_counts=counts)
    n = 300
    G, _ = synth.make_samples(founders, af, n, seed=8)
    rng = np.random.default_rng(9)
    for c in model.classifiers:
        c.samp_num = np.bincount(rng.integers(0, n, n), minlength=n).astype(np.int32)
    model.classifiers[0].samp_num[:8] = 0
    model.classifiers[9].samp_num[:8] = 0
    G[0, :] = NA_INTEGER
    G[1, model.classifiers[0].snpidx] = NA_INTEGER
    G[2, model.classifiers[9].snpidx] = NA_INTEGER
    G[3, model.classifiers[0].snpidx[::2]] = NA_INTEGER
    G[4, model.classifiers[6].snpidx[1::2]] = NA_INTEGER
    G[5, model.classifiers[10].snpidx[::3]] = NA_INTEGER
    use = (_samp_num(model) == 0).astype(np.uint8)
    use[[4, 9], 64:128] = 0                                # a whole 64-sample group uses neither: pass 1 skips both there
    use[:, list(ALL_ONES)] = 1
    use[:, list(ALL_ZEROS)] = 0
    for col, c in ((ONLY_0, 0), (ONLY_9, 9)):
        use[:, list(col)] = 0
        use[c, list(col)] = 1
    want = {v: MR.masked(model, G, use, v) for v in VOTES}
    return model, G, use, want


def test_engine_mix_and_batch_boundaries(mix_case, monkeypatch):
    model, G, use, want = mix_case
    monkeypatch.setenv("HIBAG_MASK_BATCH", "128")          # 128 + 128 + 44 samples
    dev = hb.hlaModelFromObj(model)
    kinds = {dev.engine(c) for c in range(len(model.classifiers))}
    assert ("fp4", 1) in kinds
    assert any(e == "fp4" and k > 1 for e, k in kinds)
    assert any(e == "valu" for e, _ in kinds)
    assert dev.engine(9)[0] == "valu"
    assert not use[[4, 9], 64:128].any() and use[:, 64:128].any(axis=1).sum() == len(model.classifiers) - 2
    for vote in VOTES:
        # a full-model call first: whatever it leaves in the workspace (the rows of classifiers 4 and 9 in group 1) must not leak
        dev.predict_raw(G, vote_method=vote)
        got = _masked(dev, G, use, vote)
        MR.same_bits(got, want[vote], f"vote {vote}")
        for s in ALL_ZEROS:
            assert got["h1"][s] == NA_INTEGER and got["prob"][s] == 0 and np.isnan(got["matching"][s])
    assert dev.handover_faults() == 0 and dev.status() == 0
    # one batch gives the same
    monkeypatch.delenv("HIBAG_MASK_BATCH")
    MR.same_bits(_masked(dev, G, use, 1), want[1], "one batch")
    dev.close()


def test_all_ones_mask_is_predict_raw_and_leaves_it_alone(mix_case):
    model, G, use, _ = mix_case
    dev = hb.hlaModelFromObj(model)
    ones = np.ones_like(use)
    for vote in VOTES:
        before = dev.predict_raw(G, vote, want_dosage=True, want_prob=True)
        MR.same_bits(_masked(dev, G, ones, vote), before, f"all ones, vote {vote}")
        between = dev.predict_raw(G, vote, want_dosage=True, want_prob=True)
        _masked(dev, G, use, vote)
        after = dev.predict_raw(G, vote, want_dosage=True, want_prob=True)
        MR.same_bits(between, before, "predict_raw between masked calls")
        MR.same_bits(after, before, "predict_raw after masked calls")
    # the optional outputs follow predict_raw's rules
    r = dev.predict_masked(G, use, want_dosage=False)
    assert set(r) == {"h1", "h2", "prob", "matching"}
    dev.close()


# ---- 2. every form of pass 2 ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def width_case():
    """The width sweep of tests/test_hip_parity.py::test_all_forms_of_pass_two with a random mask (p = 0.37) and one
    64-sample group in which every other classifier is unused."""
    ks = list(range(1, 41)) + [63, 64, 65, 66, 96, 127, 128]
    model, founders, af = synth.make_model("hla-a-small", seed=77, n_classifier=len(ks), n_snp=160, snp_counts=ks,
                                           wide_classifier=False)
    G, _ = synth.make_samples(founders, af, 200, seed=78, miss=0.05)
    use = (np.random.default_rng(79).random((len(ks), 200)) < 0.37).astype(np.uint8)
    use[::2, 64:128] = 0
    return model, G, use, MR.masked(model, G, use, 1)


@pytest.mark.parametrize("mode", ["stream", "hybrid", "recompute"])
def test_every_form_of_pass_two(width_case, monkeypatch, mode):
    """k_accum reads the weight from winv, k_accum_cells from cw: a weight written to one of them alone fails here."""
    model, G, use, want = width_case
    monkeypatch.setenv("HIBAG_PASS2", mode)
    if mode == "hybrid":
        monkeypatch.setenv("HIBAG_STORE_PAIRS", "3")
    dev = hb.hlaModelFromObj(model)
    assert dev.stored_cells() > 0
    assert (dev.second_pass_pairs() == 0) == (mode == "stream")
    MR.same_bits(_masked(dev, G, use, 1), want, mode)
    dev.close()


# ---- 3. both engines ------------------------------------------------------------------------------------------------

def test_both_engines(monkeypatch):
    model, founders, af = synth.make_model("hla-b", n_classifier=30)
    n = 130
    G, _ = synth.make_samples(founders, af, n)
    G[9, :] = NA_INTEGER
    use = MR.bootstrap(30, n, seed=31) == 0
    got = {}
    for engine in ("mfma", "valu"):
        monkeypatch.setenv("HIBAG_ENGINE", engine)
        dev = hb.hlaModelFromObj(model)
        assert (dev.engine(0)[0] == "valu") == (engine == "valu")
        got[engine] = _masked(dev, G, use, 1)
        dev.close()
    MR.same_bits(got["mfma"], got["valu"], "mfma against valu")
    MR.same_bits(got["mfma"], MR.masked(model, G, use, 1), "mfma")


# ---- 5. the reference's own models ----------------------------------------------------------------------------------

def _hla(table):
    return hb.HlaAlleleClass(locus="A", sample_id=list(table["sample.id"]), allele1=list(table["A.1"]), allele2=list(table["A.2"]))


@pytest.mark.parametrize("which", ["oob", "modellist_a"])
def test_reference_models_with_their_stored_bootstrap(which, model_oob, model_a, hapmap_geno, hla_type_table):
    model = model_oob if which == "oob" else model_a
    G = align_geno(model, hapmap_geno)
    sn = _samp_num(model)
    use = sn == 0
    hla = _hla(hla_type_table)
    dev = hb.hlaModelFromObj(model)
    for vote, name in zip(VOTES, ("prob", "majority")):
        want = MR.masked(model, G, use, vote)
        MR.same_bits(_masked(dev, G, use, vote), want, f"{which} vote {vote}")
        for thr in (float("nan"), 0.5):
            got = hb.hlaOutOfBagEnsemble(dev, hla, hapmap_geno, call_threshold=thr, vote=name, type="response+prob", verbose=False)
            pred = hb.HlaAlleleClass(locus=model.hla_locus, sample_id=list(model.sample_id), h1=want["h1"], h2=want["h2"],
                                     levels=model.hla_allele, prob=want["prob"])
            ref = hb.hlaCompareAllele(hla, pred, allele_limit=model, call_threshold=thr, full=True)
            assert got["overall"].keys() == ref["overall"].keys()
            for k, v in ref["overall"].items():
                assert np.array_equal(got["overall"][k], v, equal_nan=True), k
            assert np.array_equal(got["confusion"], ref["confusion"])
            assert np.array_equal(got["n_oob"], use.sum(axis=0)) and got["n_oob"].dtype == np.int32
            assert got["never_oob"] == []
            assert got["pred"].sample_id == list(model.sample_id)
            MR.same_bits({"prob": got["pred"].prob, "matching": got["pred"].matching, "postprob": got["pred"].postprob.T},
                         want, keys=("prob", "matching", "postprob"))
    dev.close()
    # from the plain object too (a model handle of the call's own), with the dosage
    got = hb.hlaOutOfBagEnsemble(model, hla, hapmap_geno, type="response+dosage", verbose=False)
    MR.same_bits({"h1": got["pred"].h1, "dosage": got["pred"].dosage.T}, MR.masked(model, G, use, 1), keys=("h1", "dosage"))


def test_a_sample_in_bag_everywhere_is_left_out(model_oob, hapmap_geno, hla_type_table):
    hla = _hla(hla_type_table)
    k = 5
    cls = [dataclasses.replace(c, samp_num=np.asarray(c.samp_num, np.int32).copy()) for c in model_oob.classifiers]
    for c in cls:
        c.samp_num[k] = 1
    model = dataclasses.replace(model_oob, classifiers=cls)
    with pytest.warns(UserWarning, match="1 training sample is in-bag in every classifier"):
        got = hb.hlaOutOfBagEnsemble(model, hla, hapmap_geno, verbose=False)
    assert got["never_oob"] == [model.sample_id[k]] and got["n_oob"][k] == 0
    assert got["pred"].h1[k] == NA_INTEGER and got["pred"].prob[k] == 0 and np.isnan(got["pred"].matching[k])
    G = align_geno(model, hapmap_geno)
    want = MR.masked(model, G, _samp_num(model) == 0, 1)
    keep = [s for s in range(len(G)) if s != k]
    pred = hb.HlaAlleleClass(locus=model.hla_locus, sample_id=[model.sample_id[s] for s in keep], h1=want["h1"][keep],
                             h2=want["h2"][keep], levels=model.hla_allele, prob=want["prob"][keep])
    ref = hb.hlaCompareAllele(hla, pred, allele_limit=model, full=True)
    assert got["overall"]["total.num.ind"] == ref["overall"]["total.num.ind"] == len(G) - 1
    for key, v in ref["overall"].items():
        assert np.array_equal(got["overall"][key], v, equal_nan=True), key
    assert np.array_equal(got["confusion"], ref["confusion"])


# ---- 6. errors ------------------------------------------------------------------------------------------------------

def test_errors(model_oob, hapmap_geno, hla_type_table):
    hla = _hla(hla_type_table)
    G = align_geno(model_oob, hapmap_geno)
    n, nc = len(G), len(model_oob.classifiers)
    dev = hb.hlaModelFromObj(model_oob)
    dev.set_timing(True)
    with pytest.raises(ValueError, match="use must be"):
        dev.predict_masked(G, np.ones((nc, n + 1), np.uint8))
    with pytest.raises(ValueError, match="use must be"):
        dev.predict_masked(G, np.ones((n, nc), np.uint8))
    with pytest.raises(TypeError):
        dev.predict_masked(G, np.ones((nc, n), np.float64))
    with pytest.raises(ValueError, match="Invalid 'vote_method'"):
        dev.predict_masked(G, np.ones((nc, n), np.uint8), vote_method=3)
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaOutOfBagEnsemble(dev, hla, hapmap_geno, vote="mean", verbose=False)
    with pytest.raises(ValueError, match="should be one of"):
        hb.hlaOutOfBagEnsemble(dev, hla, hapmap_geno, type="prob", verbose=False)
    with pytest.raises(TypeError):
        hb.hlaOutOfBagEnsemble(dev, hla, np.zeros((3, 3)), verbose=False)
    keep = [i for i, s in enumerate(hapmap_geno.sample_id) if s != model_oob.sample_id[0]]
    with pytest.raises(ValueError, match="Some of sample.id in the model do not exist in SNP genotypes."):
        hb.hlaOutOfBagEnsemble(dev, hla, hb.hlaGenoSubset(hapmap_geno, samp_sel=keep), verbose=False)
    keep = [i for i, s in enumerate(hapmap_geno.snp_id) if s != model_oob.snp_id[0]]
    with pytest.raises(ValueError, match="Some of snp.id in the model do not exist in SNP genotypes."):
        hb.hlaOutOfBagEnsemble(dev, hla, hb.hlaGenoSubset(hapmap_geno, snp_sel=keep), verbose=False)
    few = hb.hlaAlleleSubset(hla, [i for i, s in enumerate(hla.sample_id) if s != model_oob.sample_id[0]])
    with pytest.raises(ValueError, match="Some of sample.id in the model do not exist in HLA types."):
        hb.hlaOutOfBagEnsemble(dev, few, hapmap_geno, verbose=False)
    m = dataclasses.replace(model_oob, classifiers=list(model_oob.classifiers))
    m.classifiers[3] = dataclasses.replace(m.classifiers[3], samp_num=None)
    with pytest.raises(ValueError, match="There is no bootstrap sample index."):
        hb.hlaOutOfBagEnsemble(m, hla, hapmap_geno, verbose=False)
    # the C entry: NULL `use`, a bad vote, H1 without H2 -> EINVAL with a message; nothing of all this was launched
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u = np.ones((nc, n), np.uint8)
    h1 = np.empty(n, np.int32)
    assert L.hibag_hip_predict_masked(dev.handle, p(G), n, None, 1, None, None, None, None, None, None) == -1
    assert "use is NULL" in L.hibag_hip_last_error().decode()
    assert L.hibag_hip_predict_masked(dev.handle, p(G), n, p(u), 0, None, None, None, None, None, None) == -1
    assert "Invalid 'vote_method'." in L.hibag_hip_last_error().decode()
    assert L.hibag_hip_predict_masked(dev.handle, p(G), n, p(u), 1, p(h1), None, None, None, None, None) == -1
    assert L.hibag_hip_predict_masked(None, p(G), n, p(u), 1, None, None, None, None, None, None) == -1
    assert all(cnt == 0 for _, cnt in dev.get_timing().values())
    # no samples: success, nothing launched
    assert L.hibag_hip_predict_masked(dev.handle, None, 0, None, 1, None, None, None, None, None, None) == 0
    r = dev.predict_masked(G[:0], u[:, :0], want_prob=True)
    assert r["h1"].shape == (0,) and r["postprob"].shape == (0, model_oob.n_hla * (model_oob.n_hla + 1) // 2)
    assert all(cnt == 0 for _, cnt in dev.get_timing().values())
    # and a real call lands in the existing timer slots (the mask kernels under "pack")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dev.predict_masked(G, u)
    t = dev.get_timing()
    assert t["pack"][1] == 1 and t["total"][1] == 1 and t["accum"][1] == 1 and t["finish"][1] == 1
    dev.close()
