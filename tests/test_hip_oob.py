"""hlaOutOfBag on the GPU: hibag_hip_predict_oob bit-identical to the reference's per-classifier loop (one-classifier
model, hlaPredict of its out-of-bag samples) on the oracle and through the existing GPU path, and hlaOutOfBag's
averages equal to the ones computed here from that loop."""
import dataclasses

import numpy as np
import pytest

import hibag_amd as hb
from conftest import align_geno
from hibag_amd import NA_INTEGER, synth
from oracle_full import cohort, want_oob
from test_oob_host import TIE_RING_START, TIE_VARIANTS, oracle_oob, tie_calls, tie_case

pytestmark = pytest.mark.gpu


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("h1", "h2", "prob"))


def _gpu_loop(model, G):
    """The literal loop through the existing API: a one-classifier hlaModelFromObj + predict_raw(vote_method=1)."""
    C, n = len(model.classifiers), G.shape[0]
    out = {"h1": np.full((C, n), NA_INTEGER, np.int32), "h2": np.full((C, n), NA_INTEGER, np.int32), "prob": np.zeros((C, n))}
    for c, cls in enumerate(model.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        m1 = hb.hlaModelFromObj(dataclasses.replace(model, classifiers=[cls]))
        r = m1.predict_raw(G[oob], vote_method=1, want_dosage=False)
        m1.close()
        for k in ("h1", "h2", "prob"):
            out[k][c, oob] = r[k]
    return out


def _differ(a, b):
    """[(classifier, sample)] where a and b differ (NaN == NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
    return np.argwhere(~same)


def _samp_num(model):
    return np.stack([np.asarray(c.samp_num, np.int32) for c in model.classifiers])


@pytest.fixture(scope="module")
def synth_case():
    """A model with one-step FP4, multi-step FP4 and VALU (> 112 SNPs) classifiers, a seeded bootstrap, and a cohort
    with samples that miss some and all of a classifier's SNPs."""
    counts = [12, 18, 24, 30, 31, 40, 56, 84, 100, 113, 120, 128]
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(counts), snp_counts=counts)
    n = 300
    G, _ = synth.make_samples(founders, af, n, seed=8)
    rng = np.random.default_rng(9)
    for c in model.classifiers:
        c.samp_num = np.bincount(rng.integers(0, n, n), minlength=n).astype(np.int32)
    model.classifiers[0].samp_num[:8] = 0
    model.classifiers[9].samp_num[:8] = 0
    G[0, :] = NA_INTEGER                                       # every SNP missing
    G[1, model.classifiers[0].snpidx] = NA_INTEGER             # all of classifier 0's
    G[2, model.classifiers[9].snpidx] = NA_INTEGER             # all of a VALU classifier's
    G[3, model.classifiers[0].snpidx[::2]] = NA_INTEGER        # some
    G[4, model.classifiers[6].snpidx[1::2]] = NA_INTEGER
    G[5, model.classifiers[10].snpidx[::3]] = NA_INTEGER
    return model, G


def test_synthetic_engine_mix(synth_case):
    model, _ = synth_case
    dev = hb.hlaModelFromObj(model)
    kinds = {dev.engine(c) for c in range(len(model.classifiers))}
    dev.close()
    assert ("fp4", 1) in kinds
    assert any(e == "fp4" and k > 1 for e, k in kinds)
    assert any(e == "valu" for e, _ in kinds)


@pytest.mark.parametrize("which", ["oob", "modellist_a", "synthetic"])
def test_predict_oob_matches_the_oracle_loop(which, oracle, model_oob, model_a, hapmap_geno, synth_case, monkeypatch):
    if which == "synthetic":
        model, G = synth_case
        monkeypatch.setenv("HIBAG_OOB_BATCH", "128")           # 300 samples: three batches of the entry
    else:
        model = model_oob if which == "oob" else model_a
        G = align_geno(model, hapmap_geno)
    want = oracle_oob(oracle, model, G)
    dev = hb.hlaModelFromObj(model)
    got = dev.predict_oob(G, _samp_num(model))
    assert _same(got, want)
    assert _same(_gpu_loop(model, G), got)
    # the per-lane rescan (where the record log cannot settle a call) gives the same, lane for lane
    monkeypatch.setenv("HIBAG_OOB_RESCAN", "1")
    assert _same(dev.predict_oob(G, _samp_num(model)), want)
    dev.close()


@pytest.mark.parametrize("shape,n,env", [("hla-b", 10_000, {}), ("hla-b", 10_000, {"HIBAG_OOB_BATCH": "4032"}),
                                         ("hla-b", 10_000, {"HIBAG_OOB_RESCAN": "1"}), ("hla-drb1", 4096, {})])
def test_predict_oob_at_size_equals_the_oracle_loop(shape, n, env, monkeypatch):
    """The benchmark's cohorts with seeded bootstrap counts: every (classifier, sample) bit-equal to the oracle's loop.
    HIBAG_OOB_BATCH=4032: three batches (4,032 + 4,032 + 1,936 samples), the last ending inside a 64-sample group;
    HIBAG_OOB_RESCAN=1: every lane by the full walk.  At the DRB1 shape pass 1 stores every cell sum and runs its last rounds as chunks."""
    model, G, _ = cohort(shape, n)
    samp_num, want = want_oob(shape, n, boot_seed=n + 1)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = hb.hlaModelFromObj(model)
    if shape == "hla-drb1":
        assert dev.stored_cells() > 0
    got = dev.predict_oob(G, samp_num)
    assert dev.handover_faults() == 0 and dev.status() == 0
    dev.close()
    assert np.count_nonzero(got["h1"] != NA_INTEGER) > 0.3 * samp_num.size
    for k in ("h1", "h2", "prob"):
        bad = _differ(got[k], want[k])
        assert len(bad) == 0, (k, len(bad), "(classifier, sample, group):", [(int(c), int(s), int(s) // 64) for c, s in bad[:8]])


@pytest.mark.parametrize("snp_counts,seed,engine", [((10, 20, 27), 1, "fp4-1"), ((40, 84), 2, "fp4-k"), ((113, 120), 3, "valu")])
def test_t_ties(snp_counts, seed, engine, oracle):
    """Calls decided by a T-tie (tests/test_oob_host.py: the earlier of two cells that T merges wins) on each engine's
    pick: k_oob_pick from the record log (one-step FP4; ties in slot 1, in the ring after more than seven records, and
    between ring entries), k_oob_scan (several K steps), k_oob_best_valu.  predict_oob and hlaPredict of the
    one-classifier models equal the oracle."""
    model, G, samp_num, kind = tie_case(snp_counts, seed)
    dev = hb.hlaModelFromObj(model)
    for c in range(len(model.classifiers)):
        e, k = dev.engine(c)
        assert {"fp4-1": e == "fp4" and k == 1, "fp4-k": e == "fp4" and k > 1, "valu": e == "valu"}[engine], (c, e, k)
    want = oracle_oob(oracle, model, G)
    tie, called = tie_calls(oracle, model, G, want)       # the cases are ties: the oracle's call is not the raw first maximum
    kind = np.array(kind)
    for v in TIE_VARIANTS:
        assert tie[kind == v].sum() >= 5, v
    assert (tie[kind == "ring"] & (called[kind == "ring"] >= TIE_RING_START)).sum() >= 5
    assert (tie[kind == "first"] & (called[kind == "first"] == 0)).sum() >= 5
    got = dev.predict_oob(G, samp_num)
    dev.close()
    for k in ("h1", "h2", "prob"):
        bad = _differ(got[k], want[k])
        assert len(bad) == 0, (k, len(bad), [(int(c), int(s), kind[c], bool(tie[c, s])) for c, s in bad[:8]])
    assert _same(_gpu_loop(model, G), want)


def _average(model, hla, G, thr):
    """R/HIBAG.R:1336-1385 restated from the literal GPU loop and hlaCompareAllele(full=True)."""
    loop = _gpu_loop(model, G)
    names = ["call.rate", "accuracy", "sensitivity", "specificity", "ppv", "npv"]
    res = []
    for c, cls in enumerate(model.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        pred = hb.HlaAlleleClass(locus="A", sample_id=[model.sample_id[k] for k in oob], prob=loop["prob"][c, oob],
                                 h1=loop["h1"][c, oob], h2=loop["h2"][c, oob], levels=model.hla_allele)
        res.append(hb.hlaCompareAllele(hla, pred, allele_limit=model, call_threshold=thr, full=True))
    C = len(res)
    overall = {k: sum(r["overall"][k] for r in res) / C for k in res[0]["overall"]}
    conf = sum(r["confusion"] for r in res) / C
    tot, cnt = 0.0, 0.0
    for r in res:                                              # (in classifier order, like R's running sum)
        d = np.array([r["detail"][k] for k in names], np.float64)
        tot = tot + np.where(np.isnan(d), 0.0, d)
        cnt = cnt + ~np.isnan(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = tot / cnt
    return overall, conf, dict(zip(names, avg))


def _check(got, want):
    overall, conf, det = want
    assert got["overall"].keys() == overall.keys()
    for k, v in overall.items():
        assert np.array_equal(got["overall"][k], v, equal_nan=True), k
    assert np.array_equal(got["confusion"], conf)
    for k, v in det.items():
        assert np.array_equal(got["detail"][k], v, equal_nan=True), k


@pytest.mark.parametrize("thr", [float("nan"), 0.5])
def test_hlaOutOfBag_on_OutOfBag_RData(thr, model_oob, hapmap_geno, hla_type_table):
    hla = hb.HlaAlleleClass(locus="A", sample_id=list(hla_type_table["sample.id"]), allele1=list(hla_type_table["A.1"]),
                            allele2=list(hla_type_table["A.2"]))
    got = hb.hlaOutOfBag(model_oob, hla, hapmap_geno, call_threshold=thr, verbose=False)
    _check(got, _average(model_oob, hla, align_geno(model_oob, hapmap_geno), thr))
    assert got["detail"]["allele"] == list(model_oob.hla_allele)
    assert len(got["detail"]["miscall"]) == len(model_oob.hla_allele)


@pytest.mark.parametrize("thr", [float("nan"), 0.5])
def test_hlaOutOfBag_on_a_model_trained_here(thr):
    base, founders, af = synth.make_model("hla-b", seed=9, n_snp=300, n_classifier=1, wide_classifier=False)
    G, truth = synth.make_samples(founders, af, 1000, seed=10)
    snp = synth.as_snp_geno(base, G)
    hla = hb.hlaAllele(snp.sample_id, [base.hla_allele[a] for a in truth[:, 0]], [base.hla_allele[a] for a in truth[:, 1]],
                       locus="B")
    hb.set_seed(100)
    model = hb.hlaAttrBagging(hla, snp, nclassifier=100, verbose=False)
    got = hb.hlaOutOfBag(model, hla, snp, call_threshold=thr, verbose=False)
    obj = model.obj
    si = {s: i for i, s in enumerate(snp.sample_id)}
    ki = {s: i for i, s in enumerate(snp.snp_id)}
    Gm = np.ascontiguousarray(G[[si[s] for s in obj.sample_id]][:, [ki[s] for s in obj.snp_id]])
    _check(got, _average(obj, hla, Gm, thr))
    model.close()


def test_hlaOutOfBag_errors(model_oob, hapmap_geno, hla_type_table):
    hla = hb.HlaAlleleClass(locus="A", sample_id=list(hla_type_table["sample.id"]), allele1=list(hla_type_table["A.1"]),
                            allele2=list(hla_type_table["A.2"]))
    keep = [i for i, s in enumerate(hapmap_geno.sample_id) if s != model_oob.sample_id[0]]
    with pytest.raises(ValueError, match="Some of sample.id in the model do not exist in SNP genotypes."):
        hb.hlaOutOfBag(model_oob, hla, hb.hlaGenoSubset(hapmap_geno, samp_sel=keep), verbose=False)
    keep = [i for i, s in enumerate(hapmap_geno.snp_id) if s != model_oob.snp_id[0]]
    with pytest.raises(ValueError, match="Some of snp.id in the model do not exist in SNP genotypes."):
        hb.hlaOutOfBag(model_oob, hla, hb.hlaGenoSubset(hapmap_geno, snp_sel=keep), verbose=False)
    m = dataclasses.replace(model_oob, classifiers=list(model_oob.classifiers))
    m.classifiers[3] = dataclasses.replace(m.classifiers[3], samp_num=None)
    with pytest.raises(ValueError, match="There is no bootstrap sample index."):
        hb.hlaOutOfBag(m, hla, hapmap_geno, verbose=False)
    m.classifiers[3] = dataclasses.replace(model_oob.classifiers[3], samp_num=np.ones(model_oob.n_samp, np.int32))
    with pytest.raises(ValueError, match="classifier 4 has no out-of-bag sample"):
        hb.hlaOutOfBag(m, hla, hapmap_geno, verbose=False)
    dev = hb.hlaModelFromObj(model_oob)
    with pytest.raises(ValueError):
        dev.predict_oob(align_geno(model_oob, hapmap_geno), np.zeros((3, 3), np.int32))
    dev.close()
