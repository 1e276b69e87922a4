"""hlaSNPImportance on the GPU: hibag_hip_oob_knock's raw predictions bit-equal to the yardstick of
tests/importance_reference.py (the oracle's one-classifier model per (classifier, SNP) with that SNP's column NA), its
tallies equal as integers, the base rows equal to predict_oob, and hlaSNPImportance equal to the yardstick's summary."""
import numpy as np
import pytest

import curve_reference as CR
import hibag_amd as hb
import importance_reference as ref
import masked_reference as MR
from conftest import align_geno
from hibag_amd import NA_INTEGER, synth

pytestmark = pytest.mark.gpu

RAW = ("h1", "h2", "prob")


def _assert_raw(got, want):
    for k in RAW:
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (k, len(bad), "(row, sample):", [(int(r), int(s)) for r, s in bad[:8]])


@pytest.fixture(scope="module")
def bundled(oracle, model_oob, model_a, hapmap_geno, hla_type_table):
    out = {}
    for key, model in (("oob", model_oob), ("modellist_a", model_a)):
        G = align_geno(model, hapmap_geno)
        out[key] = (model, G, ref.truth_of(model, hla_type_table), ref.cached_raw(key, oracle, model, G))
    return out


@pytest.mark.parametrize("which", ["oob", "modellist_a"])
def test_bundled_models(which, bundled):
    model, G, truth, raw = bundled[which]
    sn = ref.samp_num_of(model)
    dev = hb.hlaModelFromObj(model)
    got = dev.predict_oob_knock(G, sn, truth, raw=True)
    base = dev.predict_oob(G, sn)
    assert dev.handover_faults() == 0 and dev.status() == 0
    dev.close()
    nv = raw["n_variant"]
    assert got["n_variant"] == nv and got["tally"].shape == (nv + len(model.classifiers), 5)
    assert np.array_equal(got["classifier"], raw["classifier"]) and np.array_equal(got["snp"], raw["snp"])
    _assert_raw(got, raw)
    assert np.array_equal(got["tally"], ref.knock_tally(model, raw, truth))
    for k in RAW:
        assert np.array_equal(got[k][nv:], base[k]), k


@pytest.fixture(scope="module")
def mix(oracle):
    """One-step FP4, multi-step FP4 and VALU classifiers (the mix of tests/test_hip_oob.py) on 130 samples -- three blocks,
    the last with 2 live lanes -- with a seeded bootstrap and the edge rows of the definition."""
    counts = [12, 18, 24, 30, 31, 40, 56, 84, 100, 113, 120, 128]
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(counts), snp_counts=counts)
    n = 130
    G, truth = synth.make_samples(founders, af, n, seed=8)
    truth = np.ascontiguousarray(truth, np.int32)
    rng = np.random.default_rng(9)
    for c in model.classifiers:
        c.samp_num = np.bincount(rng.integers(0, n, n), minlength=n).astype(np.int32)
    c0, c9 = model.classifiers[0], model.classifiers[9]
    c0.samp_num[:8] = 0
    c9.samp_num[:8] = 0
    model.classifiers[5].samp_num[:64] = 1                     # no out-of-bag sample in block 0: that group is skipped
    assert np.any(model.classifiers[5].samp_num[64:] == 0)
    G[0, :] = NA_INTEGER                                       # every SNP missing
    G[1, c0.snpidx[1:]] = NA_INTEGER                           # all but one SNP of classifier 0: its knock-out leaves w = 0
    G[1, c0.snpidx[0]] = 1
    G[2, c9.snpidx] = NA_INTEGER                               # all of a VALU classifier's
    G[3, c0.snpidx[::2]] = NA_INTEGER                          # already missing SNPs that get knocked out
    G[4, model.classifiers[6].snpidx[1::2]] = NA_INTEGER
    truth[6] = NA_INTEGER                                      # a sample without a truth is not counted
    model.sample_id = [f"s{i}" for i in range(n)]
    raw = ref.knock_raw(oracle, model, G, avx2=True, n_threads=8)
    for k in RAW:
        raw[k].setflags(write=False)
    return model, G, truth, raw


def test_engine_mix_case_is_what_it_says(mix):
    model, G, truth, raw = mix
    dev = hb.hlaModelFromObj(model)
    kinds = {dev.engine(c) for c in range(len(model.classifiers))}
    dev.close()
    assert ("fp4", 1) in kinds and any(e == "fp4" and k > 1 for e, k in kinds) and any(e == "valu" for e, _ in kinds)
    nv = raw["n_variant"]
    assert nv == 756
    # the lane with one typed SNP: a call in the base row, none once that SNP is knocked out, the base call otherwise
    assert raw["h1"][nv, 1] != NA_INTEGER and raw["h1"][0, 1] == NA_INTEGER and raw["prob"][0, 1] == 0.0
    assert raw["prob"][1, 1] == raw["prob"][nv, 1]
    # the lane that already misses SNP 0 of classifier 0 equals its base lane there
    assert raw["prob"][0, 3] == raw["prob"][nv, 3] and raw["h1"][nv, 3] != NA_INTEGER
    assert raw["h1"][nv, 0] == NA_INTEGER and raw["h1"][nv + 9, 2] == NA_INTEGER
    # knock-outs change calls on every engine
    t = ref.knock_tally(model, raw, truth)
    for c in (0, 7, 9):
        assert t[:nv][raw["classifier"] == c, 4].sum() > 0, c


def test_engine_mix(mix, monkeypatch):
    model, G, truth, raw = mix
    sn = ref.samp_num_of(model)
    want_tally = ref.knock_tally(model, raw, truth)
    dev = hb.hlaModelFromObj(model)
    before = dev.predict_raw(G, want_dosage=False)             # the whole model first: stale rows in the workspace
    oob_before = dev.predict_oob(G, sn)
    # the other whole-call entries share the knock-out's input and output arenas and its SNP-users index: what they return
    # before the knock-out runs, between its runs and after them is the same, bit for bit
    use = np.random.default_rng(10).integers(0, 2, (len(model.classifiers), G.shape[0])).astype(np.uint8)
    shared = lambda: (dev.predict_masked(G, use, want_dosage=True, want_prob=True), dev.predict_prefix(G, [1, 5, 12]))
    shared_runs = [shared()]
    runs = []
    for i, env in enumerate(({"HIBAG_KNOCK_BATCH": "128"}, {}, {"HIBAG_OOB_RESCAN": "1"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            runs.append(dev.predict_oob_knock(G, sn, truth, raw=True))
        # the handle is untouched between the calls
        between = dev.predict_raw(G, want_dosage=False)
        for k in ("h1", "h2", "prob", "matching"):
            assert np.array_equal(between[k], before[k], equal_nan=True), k
        if i == 0:
            shared_runs.append(shared())
    shared_runs.append(shared())
    oob_after = dev.predict_oob(G, sn)
    assert dev.handover_faults() == 0 and dev.status() == 0
    dev.close()
    # (bit for bit: the same 64 bits, or NaN in both -- the sample without a SNP has NaN in matching, dosage and posterior)
    for i, (masked, prefix) in enumerate(shared_runs[1:], 1):
        assert set(masked) == set(MR.KEYS) and set(prefix) == set(CR.KEYS)
        MR.same_bits(masked, shared_runs[0][0], f"predict_masked, call {i}")
        CR.assert_curve_equal(prefix, shared_runs[0][1], f"predict_prefix, call {i}")
    for got in runs:
        _assert_raw(got, raw)
        assert np.array_equal(got["tally"], want_tally)
    nv = raw["n_variant"]
    for k in RAW:
        assert np.array_equal(oob_before[k], oob_after[k]) and np.array_equal(runs[1][k][nv:], oob_after[k]), k


def test_threshold_and_raw_false(mix):
    model, G, truth, raw = mix
    sn = ref.samp_num_of(model)
    dev = hb.hlaModelFromObj(model)
    thr = dev.predict_oob_knock(G, sn, truth, call_threshold=0.5)
    plain = dev.predict_oob_knock(G, sn, truth)
    none = dev.predict_oob_knock(G, sn)                         # no truth: nobody is counted
    dev.close()
    assert set(thr) == {"tally", "n_variant", "classifier", "snp"}
    want = ref.knock_tally(model, raw, truth, 0.5)
    assert np.array_equal(thr["tally"], want)
    assert np.array_equal(plain["tally"], ref.knock_tally(model, raw, truth))
    assert want[:, 1].sum() < plain["tally"][:, 1].sum()        # (the threshold does leave calls out)
    assert not none["tally"].any()


def test_rejections(mix):
    model, G, truth, _ = mix
    sn = ref.samp_num_of(model)
    dev = hb.hlaModelFromObj(model)
    with pytest.raises(ValueError, match="samp_num must be"):
        dev.predict_oob_knock(G, sn[:, :-1], truth)
    with pytest.raises(ValueError, match="truth must be"):
        dev.predict_oob_knock(G, sn, truth[:-1])
    with pytest.raises(ValueError, match="genomat must be"):
        dev.predict_oob_knock(G[:, :-1], sn, truth)
    # the C entry's own checks, before any launch
    from hibag_amd import _lib
    L = _lib.lib()
    t = np.zeros((len(sn) + 756, 5), np.int64)
    p = lambda a: a.ctypes.data
    assert L.hibag_hip_oob_knock(None, p(G), G.shape[0], p(sn), p(truth), 0.0, p(t), None, None, None) == -1
    assert L.hibag_hip_oob_knock(dev.handle, p(G), -1, p(sn), p(truth), 0.0, p(t), None, None, None) == -1
    assert L.hibag_hip_oob_knock(dev.handle, None, G.shape[0], p(sn), p(truth), 0.0, p(t), None, None, None) == -1
    assert L.hibag_hip_oob_knock(dev.handle, p(G), G.shape[0], None, p(truth), 0.0, p(t), None, None, None) == -1
    assert L.hibag_hip_oob_knock(dev.handle, p(G), G.shape[0], p(sn), None, 0.0, p(t), None, None, None) == -1
    assert L.hibag_hip_oob_knock(dev.handle, p(G), G.shape[0], p(sn), p(truth), 0.0, None, None, None, None) == -1
    h = np.zeros((len(t), G.shape[0]), np.int32)
    assert L.hibag_hip_oob_knock(dev.handle, p(G), G.shape[0], p(sn), p(truth), 0.0, p(t), p(h), None, None) == -1
    assert b"together" in L.hibag_hip_last_error()
    assert dev.knock_variants() == 756
    assert dev.handover_faults() == 0 and dev.status() == 0
    dev.close()


@pytest.mark.parametrize("thr", [float("nan"), 0.5])
def test_hlaSNPImportance_on_OutOfBag_RData(thr, bundled, hapmap_geno, hla_type_table):
    model, G, truth, raw = bundled["oob"]
    hla = hb.HlaAlleleClass(locus="A", sample_id=list(hla_type_table["sample.id"]), allele1=list(hla_type_table["A.1"]),
                            allele2=list(hla_type_table["A.2"]))
    tally = ref.knock_tally(model, raw, truth, thr)
    want = ref.summary(model, tally)
    dev = hb.hlaModelFromObj(model)
    results = [hb.hlaSNPImportance(model, hla, hapmap_geno, call_threshold=thr, detail=True, verbose=False),
               hb.hlaSNPImportance(dev, hla, hapmap_geno, call_threshold=thr, verbose=False)]
    assert dev.status() == 0                                   # the open handle stays open and usable
    dev.close()
    nv = raw["n_variant"]
    for got in results:
        assert list(got.n_classifier) == want["n_classifier"] and list(got.n_used) == want["n_used"]
        for k in ("importance", "acc_base", "acc_drop", "importance_ind", "changed"):
            assert np.array_equal(getattr(got, k), np.array(want[k]), equal_nan=True), k
        assert np.array_equal(got.base_tally, tally[nv:])
        assert list(got.ranking()) == ref.ranking(want["importance"])
        assert got.snp_id == list(model.snp_id)
    assert np.array_equal(results[0].variant_tally, tally[:nv]) and results[1].variant_tally is None
    assert np.array_equal(results[0].variant_classifier, raw["classifier"]) and np.array_equal(results[0].variant_snp, raw["snp"])
    if not np.isfinite(thr):
        assert np.count_nonzero(results[0].importance > 0) >= 50
