"""The underflow and edge-case corpus (``ref_cases.PREDICT_CASES``: totals of 0 and below 1 / DBL_MAX, classifiers without
haplotypes, zero frequencies, mirrored ties, genotype values outside 0..2, and 64-sample groups that mix healthy, inf, NaN
and inactive lanes) through every entry that restates the accumulate / pick arithmetic in kernels of its own: the curve
(k_prefix_accum), out of bag (k_oob_pick, k_oob_scan, k_oob_best_valu), the knock-out, the masked driver and the merge; and
through every entry that replaces the finish with kernels of its own: top-k (k_finish_topk), draws (k_finish_draw), groups
(k_finish_groups, with and without LDS), given (k_finish_given, k_given_dosage) and family (k_family_ratios,
k_finish_family, k_family_dosage).
Every case, every sample, no tolerance: integers equal, floats the same 64 bits or NaN in both, against the references
tests/edge_corpus.py builds from the oracle alone (tests/test_edge_corpus_host.py holds the inputs to what they are for)."""

import ctypes as C

import numpy as np
import pytest

import curve_reference as CR
import edge_corpus as EC
import family_reference as FR
import given_reference as GR
import hibag_amd as hb
import importance_reference as IR
import masked_reference as MR
import ref_cases as RC
from hibag_amd import _lib

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("name", EC.CASES)
MIXED = ("mixed-lanes", "mixed-lanes-each")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


@pytest.fixture
def device_model():
    """``open(model)`` -> a device model that is checked (status 0, no hand-over fault) and closed after the test."""
    opened = []

    def open_(model):
        opened.append(hb.hlaModelFromObj(model))
        return opened[-1]
    yield open_
    for dev in opened:
        try:
            assert dev.status() == 0 and dev.handover_faults() == 0
        finally:
            dev.close()


def _rows_equal(got, want, what, keys=("h1", "h2", "prob")):
    """[rows, n_samp] outputs: integers equal, floats the same bits or NaN in both; names the first (row, sample, group)."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        if a.dtype.kind == "i":
            bad = a != b
        else:
            bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
        if bad.any():
            at = np.argwhere(bad)
            r, s = (int(v) for v in at[0])
            raise AssertionError(f"{what} {k}: {len(at)} entries differ, the first at row {r}, sample {s} (group {s // 64}, "
                                 f"lane {s % 64}): got {a[r, s]!r}, reference {b[r, s]!r}")


# ---- the curve ------------------------------------------------------------------------------------------------------------
@CASES
def test_prefix(name, device_model, monkeypatch):
    model, G = EC.case(name)
    want = EC.curve_want(name)
    dev = device_model(model)
    sizes = np.arange(1, len(model.classifiers) + 1, dtype=np.int32)
    CR.assert_curve_equal(dev.predict_prefix(G, sizes), want, name)
    assert dev.status() == 0 and dev.handover_faults() == 0
    if name in MIXED:
        monkeypatch.setenv("HIBAG_PREFIX_BATCH", "64")                    # four batches, the last of eight samples
        CR.assert_curve_equal(dev.predict_prefix(G, sizes), want, name + ", batches of 64")
        CR.assert_curve_equal(dev.predict_prefix(G, [4, 12]), {k: want[k][[3, 11]] for k in CR.KEYS}, name + ", sizes 4 and 12")


# ---- out of bag -----------------------------------------------------------------------------------------------------------
def _engine_kinds(dev, classifiers):
    kinds = {c: dev.engine(c) for c in classifiers}
    return kinds, {("valu" if e == "valu" else "one-step" if k == 1 else "k-steps") for e, k in kinds.values()}


@CASES
@pytest.mark.parametrize("boot", ["seeded", "all-out"])
def test_oob(name, boot, device_model, monkeypatch):
    model, G = EC.case(name)
    sn = EC.samp_num(name, boot)
    want = EC.oob_want(name, boot)
    dev = device_model(model)
    if name == "mixed-lanes-each":
        # a scaled classifier on each pick kernel: k_oob_pick (one K step), k_oob_scan (several), k_oob_best_valu
        kinds, picks = _engine_kinds(dev, RC.MIXED_PER_CLASSIFIER["scaled"])
        assert picks == {"one-step", "k-steps", "valu"}, kinds
    _rows_equal(dev.predict_oob(G, sn), want, f"{name}, {boot}")
    with monkeypatch.context() as mp:
        mp.setenv("HIBAG_OOB_RESCAN", "1")
        _rows_equal(dev.predict_oob(G, sn), want, f"{name}, {boot}, every lane by the full walk")
    monkeypatch.setenv("HIBAG_OOB_BATCH", "128")
    _rows_equal(dev.predict_oob(G, sn), want, f"{name}, {boot}, batches of 128")


# ---- the knock-out --------------------------------------------------------------------------------------------------------
@CASES
def test_knock(name, device_model):
    model, G, truth = EC.knock_case(name)
    raw = EC.knock_want(name)
    sn = IR.samp_num_of(model)
    dev = device_model(model)
    if name in MIXED:
        _, picks = _engine_kinds(dev, range(len(model.classifiers)))
        assert picks == {"one-step", "k-steps", "valu"}
    nv = raw["n_variant"]
    for thr in (float("nan"), 0.5):
        got = dev.predict_oob_knock(G, sn, truth, call_threshold=thr, raw=True)
        assert got["n_variant"] == nv and np.array_equal(got["classifier"], raw["classifier"]) and np.array_equal(got["snp"], raw["snp"])
        _rows_equal(got, raw, f"{name}, threshold {thr}")
        want = IR.knock_tally(model, raw, truth, thr)
        bad = np.argwhere(got["tally"] != want)
        assert len(bad) == 0, (name, thr, len(bad), "(row, column):", [(int(r), int(c)) for r, c in bad[:8]])
    _rows_equal({k: got[k][nv:] for k in ("h1", "h2", "prob")}, dev.predict_oob(G, sn), name + ": base rows against predict_oob")


# ---- the mask -------------------------------------------------------------------------------------------------------------
@CASES
@pytest.mark.parametrize("vote", [1, 2])
def test_masked(name, vote, device_model, monkeypatch):
    model, G = EC.case(name)
    use = EC.mask(name)
    dev = device_model(model)
    got = dev.predict_masked(G, use, vote, want_dosage=True, want_prob=True)
    MR.same_bits(got, EC.masked_want(name, vote), f"{name}, vote {vote}")
    if name in MIXED:
        with monkeypatch.context() as mp:
            mp.setenv("HIBAG_MASK_BATCH", "64")
            got = dev.predict_masked(G, use, vote, want_dosage=True, want_prob=True)
        MR.same_bits(got, EC.masked_want(name, vote), f"{name}, vote {vote}, batches of 64")
    ones = dev.predict_masked(G, np.ones_like(use), vote, want_dosage=True, want_prob=True)
    MR.same_bits(ones, dev.predict_raw(G, vote, want_dosage=True, want_prob=True), f"{name}, vote {vote}: all-ones mask against predict_raw")
    MR.same_bits(ones, EC.plain_want(name, vote), f"{name}, vote {vote}: all-ones mask against the oracle")


# ---- plain predict --------------------------------------------------------------------------------------------------------
@CASES
@pytest.mark.parametrize("vote", [1, 2])
def test_plain_and_resident_cohort(name, vote, device_model):
    model, G = EC.case(name)
    want = EC.plain_want(name, vote)
    dev = device_model(model)
    MR.same_bits(dev.predict_raw(G, vote, want_dosage=True, want_prob=True), want, f"{name}, vote {vote}")
    n, S = G.shape
    snp = hb.HlaSNPGeno(genotype=np.ascontiguousarray(G.T), sample_id=[f"S{i}" for i in range(n)], snp_id=[f"r{i}" for i in range(S)],
                        snp_position=np.arange(S, dtype=np.float64), snp_allele=["A/G"] * S, assembly="hg19")
    with hb.HlaDeviceCohort(snp) as coh:
        got = dev.predict_cohort(coh, np.arange(S, dtype=np.int32), None, vote, want_dosage=True, want_prob=True)
    MR.same_bits(got, want, f"{name}, vote {vote}, resident cohort")


# ---- the merge ------------------------------------------------------------------------------------------------------------
MERGE_KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")


def _merge_equal(got, want, what):
    """h1 .. matching [n]; dosage [n_hla, n] and postprob [P, n]: MR.same_bits reads the first axis as the sample."""
    MR.same_bits({k: np.asarray(got[k]).T for k in MERGE_KEYS}, {k: np.asarray(want[k]).T for k in MERGE_KEYS}, what, MERGE_KEYS)


@CASES
@pytest.mark.parametrize("use_matching", [True, False])
def test_predict_merge(name, use_matching):
    """hibag_hip_predict_merge: both models predicted and merged on the device."""
    models = EC.merge_models(name)
    _, G = EC.case(name)
    want = EC.merge_want(name, use_matching)
    devs = [hb.hlaModelFromObj(m) for m in models]
    try:
        got = hb.hlaPredictMerge(devs, np.ascontiguousarray(G.T), weight=EC.MERGE_WEIGHT, use_matching=use_matching,
                                 ret_postprob=True, verbose=False)
        for d in devs:
            assert d.status() == 0 and d.handover_faults() == 0
    finally:
        for d in devs:
            d.close()
    _merge_equal({k: getattr(got, k) for k in MERGE_KEYS}, want, f"{name}, use_matching {use_matching}")


@CASES
@pytest.mark.parametrize("use_matching", [True, False])
def test_merge_device(name, use_matching, monkeypatch):
    """hibag_hip_merge_device on the oracle's own posteriors and matching values: the merge kernels alone."""
    import torch
    plan, pp, mt = EC.merge_inputs(name)
    want = EC.merge_want(name, use_matching)
    n = pp[0].shape[1]
    nh, P, ld = len(plan.hla_allele), plan.n_row, n + 3
    dev = torch.device("cuda", 0)
    d_pp = [torch.from_numpy(np.ascontiguousarray(p.T)).to(dev) for p in pp]          # [n, n_cell_i], as predict_device writes it
    d_mt = [torch.from_numpy(np.array(m)).to(dev) for m in mt]
    maps = [np.ascontiguousarray(r, np.int32) for r in plan.row_of_cell]
    w = np.asarray(EC.MERGE_WEIGHT, np.float64)
    w = w / w.sum()
    L = _lib.lib()
    h = L.hibag_hip_merge_plan_new(2, np.array([len(r) for r in maps], np.int32).ctypes.data_as(C.c_void_p),
                                   (C.c_void_p * 2)(*[r.ctypes.data for r in maps]), nh, 0)
    assert h, L.hibag_hip_last_error()
    st = torch.cuda.current_stream(dev)
    try:
        for chunk in (None, "64"):
            if chunk:
                monkeypatch.setenv("HIBAG_MERGE_CHUNK", chunk)
            o = dict(h1=torch.empty(n, dtype=torch.int32, device=dev), h2=torch.empty(n, dtype=torch.int32, device=dev),
                     prob=torch.empty(n, dtype=torch.float64, device=dev), matching=torch.empty(n, dtype=torch.float64, device=dev),
                     dosage=torch.zeros((nh, ld), dtype=torch.float64, device=dev),
                     postprob=torch.zeros((P, ld), dtype=torch.float64, device=dev))
            _lib.check(L.hibag_hip_merge_device(
                C.c_void_p(h), (C.c_void_p * 2)(*[p.data_ptr() for p in d_pp]), (C.c_void_p * 2)(*[t.data_ptr() for t in d_mt]),
                w.ctypes.data_as(C.c_void_p), int(use_matching), n, C.c_void_p(o["h1"].data_ptr()), C.c_void_p(o["h2"].data_ptr()),
                C.c_void_p(o["prob"].data_ptr()), C.c_void_p(o["matching"].data_ptr()), C.c_void_p(o["dosage"].data_ptr()),
                C.c_void_p(o["postprob"].data_ptr()), ld, C.c_void_p(st.cuda_stream)))
            torch.cuda.synchronize(dev)
            got = {k: v.cpu().numpy() for k, v in o.items()}
            assert (got["dosage"][:, n:] == 0).all() and (got["postprob"][:, n:] == 0).all()      # nothing beyond n_samp
            got["dosage"], got["postprob"] = got["dosage"][:, :n], got["postprob"][:, :n]
            _merge_equal(got, want, f"{name}, use_matching {use_matching}, chunk {chunk}")
    finally:
        L.hibag_hip_merge_plan_free(C.c_void_p(h))


# ---- top-k, draws, groups, given, family: the finishes with kernels of their own ------------------------------------------------
VOTES = pytest.mark.parametrize("vote", [1, 2])


def _samples_equal(got, want, what, keys):
    """Outputs whose first axis is the sample: integers equal, floats the same bits or NaN in both; names the first
    differing sample with its group and lane."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind == "i":
            bad = a != b
        else:
            bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
        if bad.any():
            at = np.argwhere(bad)
            s = int(at[0][0])
            raise AssertionError(f"{what} {k}: {len(at)} entries differ, the first at sample {s} (group {s // 64}, lane {s % 64})"
                                 f"{'' if a.ndim == 1 else f', column {int(at[0][1])}'}: got {a[tuple(at[0])]!r}, "
                                 f"reference {b[tuple(at[0])]!r}")


def _clean(dev):
    assert dev.status() == 0 and dev.handover_faults() == 0


def _cohort_of(G):
    n, S = G.shape
    return hb.HlaSNPGeno(genotype=np.ascontiguousarray(G.T), sample_id=[f"S{i}" for i in range(n)], snp_id=[f"r{i}" for i in range(S)],
                         snp_position=np.arange(S, dtype=np.float64), snp_allele=["A/G"] * S, assembly="hg19")


LIST_KEYS = ("h1", "h2", "prob", "matching")


@CASES
@VOTES
def test_topk(name, vote, device_model):
    model, G = EC.case(name)
    dev = device_model(model)
    raw = dev.predict_raw(G, vote, want_dosage=False)
    called = raw["h1"] != hb.NA_INTEGER
    for k in EC.TOPK_K:
        got = dev.predict_topk(G, k, vote)
        _clean(dev)
        _samples_equal(got, EC.topk_want(name, vote, k), f"{name}, vote {vote}, k {k}", LIST_KEYS)
        _samples_equal({key: got[key][called, 0] for key in ("h1", "h2", "prob")}, {key: raw[key][called] for key in ("h1", "h2", "prob")},
                       f"{name}, vote {vote}, k {k}: rank 0 against predict_raw", ("h1", "h2", "prob"))
    if name in MIXED:
        col = np.arange(G.shape[1], dtype=np.int32)
        with hb.HlaDeviceCohort(_cohort_of(G)) as coh:
            for k in EC.TOPK_K:
                got = dev.predict_topk_cohort(coh, col, None, k, vote)
                _clean(dev)
                _samples_equal(got, EC.topk_want(name, vote, k), f"{name}, vote {vote}, k {k}, resident cohort", LIST_KEYS)


@CASES
@VOTES
def test_draws(name, vote, device_model):
    model, G = EC.case(name)
    dev = device_model(model)
    for sample0 in EC.DRAW_SAMPLE0:
        for n in EC.DRAW_N:
            got = dev.predict_draw(G, n, EC.DRAW_SEED, vote, sample0=sample0)
            _clean(dev)
            _samples_equal(got, EC.draws_want(name, vote, n, sample0), f"{name}, vote {vote}, n {n}, sample0 {sample0}", LIST_KEYS)
    if name in MIXED:
        col = np.arange(G.shape[1], dtype=np.int32)
        with hb.HlaDeviceCohort(_cohort_of(G)) as coh:
            for n in EC.DRAW_N:
                got = dev.predict_draw_cohort(coh, col, None, n, EC.DRAW_SEED, vote, sample0=EC.DRAW_SAMPLE0[1])
                _clean(dev)
                _samples_equal(got, EC.draws_want(name, vote, n, EC.DRAW_SAMPLE0[1]), f"{name}, vote {vote}, n {n}, resident cohort", LIST_KEYS)


GROUP_KEYS = ("g1", "g2", "prob", "matching", "dosage")


@CASES
@VOTES
def test_groups(name, vote, device_model, monkeypatch):
    model, G = EC.case(name)
    want = EC.groups_want(name, vote)
    nh = EC.n_hla(name)
    dev = device_model(model)
    raw = dev.predict_raw(G, vote, want_dosage=True)
    with dev.groups_plan(EC.partitions(name)) as plan:
        assert plan.tile()[1] is True
        got = dev.predict_groups(G, plan, vote, want_dosage=True)
        _clean(dev)
        _samples_equal(got, want, f"{name}, vote {vote}", GROUP_KEYS)
        lean = dev.predict_groups(G, plan, vote, want_dosage=False)
        _samples_equal(lean, want, f"{name}, vote {vote}, no dosage", GROUP_KEYS[:4])
        # the identity partition is the plain finish
        mine = {"h1": got["g1"][:, EC.IDENTITY], "h2": got["g2"][:, EC.IDENTITY], "prob": got["prob"][:, EC.IDENTITY],
                "dosage": got["dosage"][:, :nh]}
        _samples_equal(mine, raw, f"{name}, vote {vote}: identity partition against predict_raw", ("h1", "h2", "prob", "dosage"))
        if name in MIXED:
            with monkeypatch.context() as mp:
                mp.setenv("HIBAG_GROUPS_NO_LDS", "1")
                assert plan.tile()[1] is False
                got = dev.predict_groups(G, plan, vote, want_dosage=True)
            _clean(dev)
            _samples_equal(got, want, f"{name}, vote {vote}, without LDS", GROUP_KEYS)
            col = np.arange(G.shape[1], dtype=np.int32)
            with hb.HlaDeviceCohort(_cohort_of(G)) as coh:
                got = dev.predict_groups_cohort(coh, col, None, plan, vote, want_dosage=True)
            _clean(dev)
            _samples_equal(got, want, f"{name}, vote {vote}, resident cohort", GROUP_KEYS)


GIVEN_KEYS = ("h1", "h2", "prob", "support", "matching", "dosage")


@CASES
@VOTES
def test_given(name, vote, device_model):
    model, G = EC.case(name)
    dev = device_model(model)
    raw = dev.predict_raw(G, vote, want_dosage=True)
    for which in EC.GIVEN_SETS:
        allow = GR.pack(EC.given_sets(name, which))
        got = dev.predict_given(G, allow, vote, want_dosage=True)
        _clean(dev)
        _samples_equal(got, EC.given_want(name, vote, which), f"{name}, vote {vote}, sets {which}", GIVEN_KEYS)
        lean = dev.predict_given(G, allow, vote, want_dosage=False)
        _samples_equal(lean, got, f"{name}, vote {vote}, sets {which}, no dosage", GIVEN_KEYS[:5])
        if which == "full":                                   # the plain finish, and the draws' S
            _samples_equal(got, raw, f"{name}, vote {vote}: full sets against predict_raw", ("h1", "h2", "prob", "dosage"))
            _samples_equal(got, {"support": EC.draw_S(name, vote)}, f"{name}, vote {vote}: full sets against S", ("support",))
    if name in MIXED:
        col = np.arange(G.shape[1], dtype=np.int32)
        with hb.HlaDeviceCohort(_cohort_of(G)) as coh:
            for which in EC.GIVEN_SETS:
                got = dev.predict_given_cohort(coh, col, None, GR.pack(EC.given_sets(name, which)), vote, want_dosage=True)
                _clean(dev)
                _samples_equal(got, EC.given_want(name, vote, which), f"{name}, vote {vote}, sets {which}, resident cohort", GIVEN_KEYS)


@CASES
@VOTES
def test_family(name, vote, device_model, monkeypatch):
    model, _ = EC.case(name)
    G = EC.family_geno(name)
    _, ped = EC.family_case(name)
    dev = device_model(model)
    raw = dev.predict_raw(G, vote, want_dosage=True)
    S = EC.draw_S(name, vote)[EC.family_case(name)[0]]
    for with_prior in (True, False):
        prior = EC.family_prior(name, with_prior)
        want = EC.family_want(name, vote, with_prior)
        got = dev.predict_family(G, ped, prior, vote, want_dosage=True)
        _clean(dev)
        _samples_equal(got, want, f"{name}, vote {vote}, prior {with_prior}", GIVEN_KEYS)
        lean = dev.predict_family(G, ped, prior, vote, want_dosage=False)
        _samples_equal(lean, want, f"{name}, vote {vote}, prior {with_prior}, no dosage", GIVEN_KEYS[:5])
        if name in MIXED:                                     # parents and children in different slices
            with monkeypatch.context() as mp:
                mp.setenv("HIBAG_STAGED_SLICE", "64")
                got = dev.predict_family(G, ped, prior, vote, want_dosage=True)
            _clean(dev)
            _samples_equal(got, want, f"{name}, vote {vote}, prior {with_prior}, slices of 64", GIVEN_KEYS)
        # founders only: the plain finish, and the draws' S
        got = dev.predict_family(G, FR.founders_only(len(G)), prior, vote, want_dosage=True)
        _clean(dev)
        _samples_equal(got, raw, f"{name}, vote {vote}, prior {with_prior}: founders against predict_raw", ("h1", "h2", "prob", "dosage"))
        _samples_equal(got, {"support": S}, f"{name}, vote {vote}, prior {with_prior}: founders against S", ("support",))


def test_wrappers_hand_infinite_probabilities_through(device_model):
    """hlaPredictTopK, hlaPredictDraws, hlaPredictGroups, hlaPredictGiven and hlaPredictFamily on subnormal-lanes: no
    exception, and the inf probabilities as the device wrote them."""
    import warnings
    name = "subnormal-lanes"
    model, G = EC.case(name)
    dev = device_model(model)
    snp = np.ascontiguousarray(G.T)
    inf = np.isposinf(EC.plain_want(name, 1)["prob"])
    assert inf.sum() >= 10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # ("No prediction output" for the samples that type nothing)
        top = hb.hlaPredictTopK(dev, snp, k=5, verbose=False)
        draws = hb.hlaPredictDraws(dev, snp, n=17, seed=EC.DRAW_SEED, verbose=False)
        groups = hb.hlaPredictGroups(dev, snp, EC.partitions(name), verbose=False)
        given = hb.hlaPredictGiven(dev, snp, EC.given_sets(name, "moved"), dosage=True, verbose=False)
        fam_G = np.ascontiguousarray(EC.family_geno(name).T)
        family = hb.hlaPredictFamily(dev, fam_G, EC.family_case(name)[1], prior="model", dosage=True, verbose=False)
    _clean(dev)
    _samples_equal({"h1": top.h1, "h2": top.h2, "prob": top.prob, "matching": top.matching}, EC.topk_want(name, 1, 5), "hlaPredictTopK", LIST_KEYS)
    assert np.isposinf(top.prob[inf]).all() and np.isposinf(top.best().prob[inf]).all()
    _samples_equal({"h1": draws.h1, "h2": draws.h2, "prob": draws.prob, "matching": draws.matching}, EC.draws_want(name, 1, 17, 0),
                   "hlaPredictDraws", LIST_KEYS)
    assert np.isposinf(draws.prob[inf]).all()
    _samples_equal({"g1": groups.g1, "g2": groups.g2, "prob": groups.prob, "matching": groups.matching, "dosage": groups.dosage},
                   EC.groups_want(name, 1), "hlaPredictGroups", GROUP_KEYS)
    assert np.isposinf(groups.prob[inf]).all()
    want = EC.given_want(name, 1, "moved")
    _samples_equal({"h1": given.h1, "h2": given.h2, "prob": given.prob_joint, "support": given.support, "matching": given.matching},
                   want, "hlaPredictGiven", GIVEN_KEYS[:5])
    assert np.isposinf(given.prob_joint[inf]).all() and np.isposinf(given.support[inf]).all()
    assert np.array_equal(given.prob, GR.conditional(want)["prob"], equal_nan=True)
    want = EC.family_want(name, 1, True)
    assert np.array_equal(hb.hlaModelAllelePrior(model), EC.family_prior(name, True))
    _samples_equal({"h1": family.h1, "h2": family.h2, "prob": family.prob_joint, "support": family.support, "matching": family.matching},
                   want, "hlaPredictFamily", GIVEN_KEYS[:5])
    assert np.isposinf(want["prob"]).sum() >= 10 and np.array_equal(family.prob, FR.conditional(want)["prob"], equal_nan=True)
