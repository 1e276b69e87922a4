"""hlaPredictMerge on the GPU: bit-identical, field by field, to hlaPredMerge(*[hlaPredict(m, snp, type="response+prob")])
computed in the same test -- every sample compared, float64 fields by their bit patterns (NaNs must match too)."""

import ctypes as C
import dataclasses
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predmerge_reference as R  # noqa: E402
from test_predmerge_host import same_bits  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import _lib, synth  # noqa: E402
from hibag_amd.merge import merge_plan  # noqa: E402

pytestmark = pytest.mark.gpu

# (seed, alleles, renamed alleles): the sets overlap without being equal
SPECS = [(11, 14, {}), (12, 11, {0: "01:09", 5: "30:01"}), (13, 16, {2: "30:01", 15: "31:02N"}), (14, 9, {8: "01:09"})]
EQUIV = {"30:01": "01:01", "31:02N": "02:02"}


def make_models(k, n_snp=80):
    objs, devs, first = [], [], None
    for seed, n_hla, ren in SPECS[:k]:
        obj, founders, afreq = synth.make_model("hla-a-small", seed=seed, n_hla=n_hla, n_snp=n_snp)
        obj.hla_allele = [ren.get(i, a) for i, a in enumerate(obj.hla_allele)]
        obj.hla_locus = "A"
        if first is None:
            first = (founders, afreq)
        objs.append(obj)
        devs.append(hb.hlaModelFromObj(obj))
    return objs, devs, first


def cohort(first, n_samp):
    geno, _ = synth.make_samples(first[0], first[1], n_samp)
    geno[n_samp // 2, :] = hb.NA_INTEGER                   # one sample with every SNP missing
    return geno


def composed(devs, snp, vote="prob", **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pds = [hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False) for m in devs]
    return hb.hlaPredMerge(*pds, verbose=False, **kw), pds


def assert_same(got, want, ret_dosage=True, ret_postprob=False, skip_dosage=False):
    assert got.locus == want.locus and list(got.sample_id) == list(want.sample_id) and got.assembly == want.assembly
    assert np.array_equal(got.h1, want.h1) and np.array_equal(got.h2, want.h2)
    assert got.allele1 == want.allele1 and got.allele2 == want.allele2
    assert same_bits(got.prob, want.prob) and same_bits(got.matching, want.matching)
    if ret_dosage:
        if not skip_dosage:
            assert same_bits(got.dosage, want.dosage)
    else:
        assert got.dosage is None and want.dosage is None
    if ret_postprob:
        assert same_bits(got.postprob, want.postprob) and got.pair_names == want.pair_names
    else:
        assert got.postprob is None and want.postprob is None


def check_status(devs):
    for m in devs:
        assert m.status() == 0


def close(devs):
    for m in devs:
        m.close()


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("n_samp", [63, 64, 65, 1000])
def test_equals_composed(k, n_samp):
    objs, devs, first = make_models(k)
    snp = synth.as_snp_geno(objs[0], cohort(first, n_samp))
    weights = [None] if k == 1 else [None, [0.7, 0.1, 1.9, 0.4][:k]]
    for weight in weights:
        for use_matching in (True, False):
            kw = dict(weight=weight, use_matching=use_matching, ret_postprob=True)
            want, _ = composed(devs, snp, **kw)
            got = hb.hlaPredictMerge(devs, snp, verbose=False, **kw)
            assert_same(got, want, True, True)
            check_status(devs)
    assert not np.isnan(want.prob).all() and len(set(want.allele1)) > 1          # the calls are not all the same
    close(devs)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_options(k):
    objs, devs, first = make_models(k)
    snp = synth.as_snp_geno(objs[0], cohort(first, 200), order="F")
    for kw in (dict(ret_dosage=False), dict(ret_dosage=False, ret_postprob=True), dict(ret_postprob=True),
               dict(max_resolution="2-digit", ret_postprob=True), dict(equivalence=EQUIV, ret_postprob=True),
               dict(equivalence=EQUIV, max_resolution="4-digit", rm_suffix=True, use_matching=False, ret_postprob=True)):
        want, _ = composed(devs, snp, **kw)
        got = hb.hlaPredictMerge(devs, snp, verbose=False, **kw)
        assert_same(got, want, kw.get("ret_dosage", True), kw.get("ret_postprob", False))
        check_status(devs)
    want, _ = composed(devs, snp, vote="majority", ret_postprob=True)
    got = hb.hlaPredictMerge(devs, snp, vote="majority", ret_postprob=True, verbose=False)
    assert_same(got, want, True, True)
    check_status(devs)
    # a bare matrix [n.snp, n.samp] (every model has the same SNP count)
    mat = np.asarray(snp.genotype)
    want, _ = composed(devs, mat, ret_postprob=True)
    got = hb.hlaPredictMerge(devs, mat, ret_postprob=True, verbose=False)
    assert_same(got, want, True, True)
    close(devs)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_one_sample(k):
    """One sample: every field the composed route's except the dosage, which is held to the plain-loop reference
    (hlaPredMerge's numpy column sum of a one-column matrix is pairwise, not in row order)."""
    objs, devs, first = make_models(k)
    geno, _ = synth.make_samples(first[0], first[1], 8)
    snp = synth.as_snp_geno(objs[0], geno[3:4])
    want, pds = composed(devs, snp, ret_postprob=True)
    got = hb.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False)
    assert_same(got, want, True, True, skip_dosage=True)
    plan = merge_plan([o.hla_allele for o in objs])
    ref = R.merge_reference([p.postprob for p in pds], [p.matching for p in pds], None, plan.row_of_cell, len(plan.hla_allele))
    assert same_bits(got.dosage, ref["dosage"]) and same_bits(got.postprob, ref["postprob"])
    assert same_bits(got.prob, ref["prob"]) and same_bits(got.matching, ref["matching"])
    check_status(devs)
    close(devs)


def test_chunked_equals_unchunked(monkeypatch):
    objs, devs, first = make_models(4)
    snp = synth.as_snp_geno(objs[0], cohort(first, 1000))
    whole = hb.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False)
    monkeypatch.setenv("HIBAG_MERGE_CHUNK", "192")          # six chunks, the last of 40 samples
    parts = hb.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False)
    monkeypatch.delenv("HIBAG_MERGE_CHUNK")
    assert_same(parts, whole, True, True)
    want, _ = composed(devs, snp, ret_postprob=True)
    assert_same(parts, want, True, True)
    check_status(devs)
    close(devs)


def test_different_snp_sets_and_bed(tmp_path):
    """One model built on a subset of the other's SNPs; the cohort as an HlaSNPGeno (both memory orders, and with more SNPs
    than the models use, which makes the host hand over the used rows only) and as a lazily opened BED file."""
    obj_a, fa, qa = synth.make_model("hla-a-small", seed=21, n_hla=12, n_snp=80)
    obj_b, _, _ = synth.make_model("hla-a-small", seed=22, n_hla=10, n_snp=50)          # SNPs 0..49 of model a's
    obj_b.hla_allele = [{1: "30:01"}.get(i, a) for i, a in enumerate(obj_b.hla_allele)]
    obj_a.hla_locus = obj_b.hla_locus = "A"
    devs = [hb.hlaModelFromObj(obj_b), hb.hlaModelFromObj(obj_a)]
    geno = cohort((fa, qa), 300)
    for order in ("C", "F"):
        snp = synth.as_snp_geno(obj_a, geno, order=order)
        want, _ = composed(devs, snp, ret_postprob=True)
        assert_same(hb.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False), want, True, True)
    # a cohort of 400 SNPs of which the models use the 80 in the middle, in reverse order
    rng = np.random.default_rng(3)
    big = rng.integers(0, 3, (400, 300)).astype(np.int32)
    big[160:240] = geno.T[::-1]
    pos = np.concatenate([np.arange(160) * 7.0 + 1000, obj_a.snp_position[::-1], np.arange(160) * 7.0 + 90_000_000])
    snp = hb.HlaSNPGeno(genotype=big, sample_id=[f"S{i}" for i in range(300)], snp_id=[f"x{i}" for i in range(400)],
                        snp_position=pos, snp_allele=["A/G"] * 400, assembly="hg19")
    want, _ = composed(devs, snp, ret_postprob=True)
    assert_same(hb.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False), want, True, True)
    bed = synth.as_bed_geno(obj_a, geno, str(tmp_path / "cohort.bed"))
    want, _ = composed(devs, bed, ret_postprob=True)
    assert_same(hb.hlaPredictMerge(devs, bed, ret_postprob=True, verbose=False), want, True, True)
    check_status(devs)
    close(devs)


def test_merge_device_on_device_buffers():
    """hibag_hip_merge_device on the buffers hibag_hip_predict_device filled equals the host-pointer entry."""
    import torch
    objs, devs, first = make_models(3)
    n = 333
    geno = cohort(first, n)
    w = np.array([0.5, 0.2, 0.3])
    want = hb.hlaPredictMerge(devs, synth.as_snp_geno(objs[0], geno), weight=w, ret_postprob=True, verbose=False)
    dev = torch.device("cuda", devs[0].device())
    d_geno = torch.from_numpy(geno).to(dev)
    pp = [torch.empty((n, o.n_cell), dtype=torch.float64, device=dev) for o in objs]
    mt = [torch.empty(n, dtype=torch.float64, device=dev) for _ in objs]
    st = torch.cuda.current_stream(dev)
    for m, p, t in zip(devs, pp, mt):
        m.predict_device(d_geno.data_ptr(), n, 1, d_matching=t.data_ptr(), d_postprob=p.data_ptr(), stream=st.cuda_stream)
    plan = merge_plan([o.hla_allele for o in objs])
    nh, P, ld = len(plan.hla_allele), plan.n_row, n + 5
    maps = [np.ascontiguousarray(r, np.int32) for r in plan.row_of_cell]
    L = _lib.lib()
    h = L.hibag_hip_merge_plan_new(3, np.array([len(r) for r in maps], np.int32).ctypes.data_as(C.c_void_p),
                                   (C.c_void_p * 3)(*[r.ctypes.data for r in maps]), nh, devs[0].device())
    assert h, L.hibag_hip_last_error()
    o = dict(h1=torch.empty(n, dtype=torch.int32, device=dev), h2=torch.empty(n, dtype=torch.int32, device=dev),
             prob=torch.empty(n, dtype=torch.float64, device=dev), matching=torch.empty(n, dtype=torch.float64, device=dev),
             dosage=torch.zeros((nh, ld), dtype=torch.float64, device=dev), postprob=torch.zeros((P, ld), dtype=torch.float64, device=dev))
    try:
        for chunk in (None, "128"):
            if chunk:
                os.environ["HIBAG_MERGE_CHUNK"] = chunk
            try:
                _lib.check(L.hibag_hip_merge_device(
                    C.c_void_p(h), (C.c_void_p * 3)(*[p.data_ptr() for p in pp]), (C.c_void_p * 3)(*[t.data_ptr() for t in mt]),
                    (w / w.sum()).ctypes.data_as(C.c_void_p), 1, n, C.c_void_p(o["h1"].data_ptr()), C.c_void_p(o["h2"].data_ptr()),
                    C.c_void_p(o["prob"].data_ptr()), C.c_void_p(o["matching"].data_ptr()), C.c_void_p(o["dosage"].data_ptr()),
                    C.c_void_p(o["postprob"].data_ptr()), ld, C.c_void_p(st.cuda_stream)))
            finally:
                os.environ.pop("HIBAG_MERGE_CHUNK", None)
            torch.cuda.synchronize(dev)
            assert np.array_equal(o["h1"].cpu().numpy(), want.h1) and np.array_equal(o["h2"].cpu().numpy(), want.h2)
            assert same_bits(o["prob"].cpu().numpy(), want.prob) and same_bits(o["matching"].cpu().numpy(), want.matching)
            assert same_bits(o["dosage"].cpu().numpy()[:, :n], want.dosage)
            assert same_bits(o["postprob"].cpu().numpy()[:, :n], want.postprob)
            assert (o["dosage"].cpu().numpy()[:, n:] == 0).all()             # nothing written beyond n_samp
    finally:
        L.hibag_hip_merge_plan_free(C.c_void_p(h))
    check_status(devs)
    close(devs)


def test_same_model_twice():
    objs, devs, first = make_models(2)
    snp = synth.as_snp_geno(objs[0], cohort(first, 100))
    lst = [devs[0], devs[1], devs[0]]
    want, _ = composed(lst, snp, ret_postprob=True)
    assert_same(hb.hlaPredictMerge(lst, snp, ret_postprob=True, verbose=False), want, True, True)
    check_status(devs)
    close(devs)


def test_errors_on_device():
    objs, devs, first = make_models(2)
    snp = synth.as_snp_geno(objs[0], cohort(first, 10))
    other = hb.hlaModelFromObj(objs[1])
    other.obj = dataclasses.replace(objs[1], hla_locus="B")
    with pytest.raises(ValueError, match="The locus should be the same."):
        hb.hlaPredictMerge([devs[0], other], snp, verbose=False)
    other.close()
    check_status(devs)
    close(devs)


def test_models_on_different_devices():
    if _lib.lib().hibag_hip_device_count() < 2:
        pytest.skip("needs two devices")
    objs, devs, first = make_models(2)
    snp = synth.as_snp_geno(objs[0], cohort(first, 10))
    far = devs[1].replicate(1)
    with pytest.raises(ValueError, match="same device"):
        hb.hlaPredictMerge([devs[0], far], snp, verbose=False)
    far.close()
    close(devs)
