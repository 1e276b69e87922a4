"""hlaPredictGroups on the GPU: hibag_hip_predict_groups and its routes equal, every sample, every partition and both vote
methods, to the reference (tests/groups_reference.py: the contract of DESIGN.md section 17 applied to the CPU oracle's
posterior matrix); the identity partition is predict_raw's own call, probability and dosage; independent of batches, slices,
routes, a repaired hand-over, the other partitions of the call and of whether dosages were asked for; the model's other
outputs untouched; invalid arguments rejected.  Every comparison is exact equality (NaN == NaN) except the cross-check with
hlaPredictMerge, whose bound is derived there."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import hibag_amd as hb
from conftest import REFDATA, align_geno
from groups_reference import assert_groups_equal, groups, groups_from_postprob, levels_of
from hibag_amd import NA_INTEGER, _lib, synth
from hibag_amd._lib import GROUPS_MAX_LEVELS, GROUPS_MAX_PART

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def identity(n_hla):
    return np.arange(n_hla, dtype=np.int32)[None, :]


def random_partitions(n_hla, sizes, seed):
    """One partition per entry of `sizes`: every allele in one of G groups at random (an id may stay unused)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, int(G), n_hla) for G in sizes]).astype(np.int32)


def gather(ref, parts, idx):
    """The reference of the partitions parts[idx] out of the reference `ref` of `parts`."""
    off = np.concatenate([[0], np.cumsum(levels_of(parts))])
    out = {k: np.ascontiguousarray(ref[k][:, idx]) for k in ("g1", "g2", "prob")}
    out["dosage"] = np.ascontiguousarray(np.concatenate([ref["dosage"][:, off[i]:off[i + 1]] for i in idx], axis=1))
    out["matching"] = ref["matching"]
    return out


def check_against_raw(got, raw, what=""):
    assert np.array_equal(got["matching"], raw["matching"], equal_nan=True), what
    na = got["g1"] == NA
    assert np.array_equal(na, got["g2"] == NA), what
    assert np.all(got["g1"][~na] <= got["g2"][~na]) and np.all(got["g1"][~na] >= 0) and np.all(got["prob"][~na] > 0), what
    assert np.all(na[raw["h1"] == NA]), what


def run_case(model, G, parts, votes=(1, 2), what="", refs=None, want_dosage=True):
    """predict_groups against the reference; returns {vote: (got, want)}."""
    out = {}
    dev = hb.hlaModelFromObj(model)
    try:
        with dev.groups_plan(parts) as plan:
            assert plan.n_part == len(parts) and np.array_equal(plan.levels, levels_of(parts))
            for vote in votes:
                got = dev.predict_groups(G, plan, vote, want_dosage=want_dosage)
                raw = dev.predict_raw(G, vote, want_dosage=False)
                assert dev.status() == 0 and dev.handover_faults() == 0
                want = refs[vote] if refs is not None else groups(model, G, parts, vote=vote)
                assert got["g1"].shape == (len(G), len(parts)) and got["g1"].dtype == np.int32 and got["prob"].dtype == np.float64
                assert ("dosage" in got) == want_dosage
                assert_groups_equal(got, want, f"{what} vote={vote}")
                check_against_raw(got, raw, f"{what} vote={vote}")
                out[vote] = (got, want)
    finally:
        dev.close()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_fixture_models_on_the_hapmap_genotypes(which, request, hapmap_geno):
    model = request.getfixturevalue(which)
    n = model.n_hla
    G = align_geno(model, hapmap_geno, hapmap_geno.sample_id)
    two_digit = hb.hlaGroupsByResolution(model.hla_allele, "2-digit").group_of
    parts = np.concatenate([identity(n), two_digit, np.zeros((1, n), np.int32),
                            random_partitions(n, np.linspace(2, n, 5).astype(int), seed=3)])
    dev = hb.hlaModelFromObj(model)
    try:
        raws = {vote: dev.predict_raw(G, vote, want_dosage=True) for vote in (1, 2)}
    finally:
        dev.close()
    for vote, (got, want) in run_case(model, G, parts, what=which).items():
        raw = raws[vote]
        # the identity partition is the model's own prediction (contract rule 5)
        for key, mine in (("h1", got["g1"][:, 0]), ("h2", got["g2"][:, 0]), ("prob", got["prob"][:, 0]),
                          ("dosage", got["dosage"][:, :n])):
            assert np.array_equal(mine, raw[key], equal_nan=True), (which, vote, key)
        # one group: one bin, the running sum of all cells
        ok = got["g1"][:, 2] != NA
        assert np.all(got["g1"][ok, 2] == 0) and np.all(got["g2"][ok, 2] == 0)
        assert np.array_equal(got["prob"][:, 2], np.where(ok, np.cumsum(want["postprob"], axis=1)[:, -1], 0.0))


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread_case():
    """tests/test_groups_host.py's corner: 14 alleles, 105 cells, 85 % of the genotypes missing, 130 samples, sample 77 with
    every SNP missing.  Six base partitions; the reference is made once per vote."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.85)
    G[77, :] = NA
    h = np.arange(model.n_hla)
    base = np.concatenate([np.stack([h % 3, h // 2, h % 2]).astype(np.int32), identity(model.n_hla),
                           random_partitions(model.n_hla, [4, 9], seed=21)])
    refs = {vote: groups(model, G, base, vote=vote) for vote in (1, 2)}
    return model, G, base, refs


# The threads of a workgroup (256: four wavefronts of 64) take the (sample of the tile, partition) pairs, partition fastest,
# tile = max(1, min(64, 256 // Q, what fits in LDS)): Q = 1 (a wavefront is 64 samples), 63 / 64 / 65 (a wavefront holds a
# sample's partitions just not / exactly / not any more; 4, 4 and 3 samples per workgroup), 129 (above twice that: one
# sample per workgroup from here on), 255 / 256 / 257 (one round of the workgroup's threads just not / exactly / not any
# more), 512 = the limit (two full rounds).
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 129, 255, 256, 257, GROUPS_MAX_PART])
def test_spread_posteriors_at_every_bound_of_the_lane_mapping(Q, spread_case):
    model, G, base, refs = spread_case
    idx = np.resize(np.random.default_rng(Q).permutation(len(base)), Q)
    if Q == 1:
        idx = np.array([0])
    parts = base[idx]
    assert levels_of(parts).sum() <= GROUPS_MAX_LEVELS
    want = {vote: gather(refs[vote], base, idx) for vote in (1, 2)}
    on = run_case(model, G, parts, what=f"spread Q={Q}", refs=want)
    off = run_case(model, G, parts, votes=(1,), what=f"spread Q={Q}, no dosage", refs=want, want_dosage=False)
    for key in ("g1", "g2", "prob", "matching"):
        assert np.array_equal(on[1][0][key], off[1][0][key], equal_nan=True), key
    for vote, (got, _) in on.items():
        assert np.all(got["g1"][77] == NA) and np.all(got["g2"][77] == NA) and np.all(got["prob"][77] == 0.0), vote
        assert np.isnan(got["matching"][77]) and np.all(got["dosage"][77] == 0.0), vote
    # the collapsed call is not the relabelled one (tests/test_groups_host.py pins the corner on the reference)
    if Q == 1:
        got = on[1][0]
        a, b = parts[0][np.maximum(refs[1]["call"]["h1"], 0)], parts[0][np.maximum(refs[1]["call"]["h2"], 0)]
        ok = refs[1]["call"]["h1"] != NA
        assert np.count_nonzero(ok & ((np.minimum(a, b) != got["g1"][:, 0]) | (np.maximum(a, b) != got["g2"][:, 0]))) >= 10


# 5 ---------------------------------------------------------------------------------------------------------------
def test_forced_direct_path_gives_the_same_arrays(spread_case, monkeypatch):
    model, G, base, refs = spread_case
    dev = hb.hlaModelFromObj(model)
    try:
        with dev.groups_plan(base) as plan:
            assert plan.tile()[1] is True
            staged = dev.predict_groups(G, plan, 1)
            monkeypatch.setenv("HIBAG_GROUPS_NO_LDS", "1")
            assert plan.tile()[1] is False
            direct = {vote: dev.predict_groups(G, plan, vote) for vote in (1, 2)}
            monkeypatch.delenv("HIBAG_GROUPS_NO_LDS")
            assert plan.tile()[1] is True
        assert dev.status() == 0
    finally:
        dev.close()
    for vote in (1, 2):
        assert_groups_equal(direct[vote], refs[vote], f"direct path vote={vote}")
    for key in staged:
        assert np.array_equal(staged[key], direct[1][key], equal_nan=True), key


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hla_b_case():
    """1,275 cells; 300 samples (not a multiple of 64), sample 0 with every SNP missing; 40 random partitions, G = 1 .. 50."""
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 300)
    G[0, :] = NA
    parts = random_partitions(model.n_hla, np.linspace(1, model.n_hla, 40).astype(int), seed=5)
    return model, G, parts


def test_hla_b_forty_partitions(hla_b_case):
    model, G, parts = hla_b_case
    assert model.n_cell == 1275 and levels_of(parts).min() == 1 and levels_of(parts).max() >= 45
    for vote, (got, _) in run_case(model, G, parts, what="hla-b").items():
        assert np.all(got["g1"][0] == NA) and np.all(got["prob"][0] == 0.0), vote


# 4 ---------------------------------------------------------------------------------------------------------------
def test_drb1_shape_and_the_models_own_prediction_is_untouched():
    """The large-n_cell, store-every-cell layout (pass 2 = k_accum_cells): 1,830 cells, four samples fit in LDS."""
    model, founders, af = synth.make_model("hla-drb1", n_classifier=8)
    G, _ = synth.make_samples(founders, af, 200)
    G[7, :] = NA
    n = model.n_hla
    parts = np.concatenate([identity(n), (np.arange(n) % 3)[None, :].astype(np.int32), random_partitions(n, [5, 31], seed=9)])
    dev = hb.hlaModelFromObj(model)
    try:
        assert dev.stored_cells() > 0 and dev.second_pass_pairs() == 0
        before = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        with dev.groups_plan(parts) as plan:
            assert plan.tile() == (min(64, 256 // len(parts), 8064 // model.n_cell), True) and plan.tile()[0] == 4
            for vote in (1, 2):
                got = dev.predict_groups(G, plan, vote)
                assert_groups_equal(got, groups(model, G, parts, vote=vote), f"drb1 vote={vote}")
                check_against_raw(got, dev.predict_raw(G, vote, want_dosage=False), f"drb1 vote={vote}")
        after = dev.predict_raw(G, 1, want_dosage=True, want_prob=True)
        assert dev.status() == 0
    finally:
        dev.close()
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key


# 6 ---------------------------------------------------------------------------------------------------------------
def two_allele_case():
    c1 = hb.Classifier([0, 1, 2, 3], [0.3, 0.3, 0.4], [0, 1, 1], ["0000", "0101", "1111"])
    c2 = hb.Classifier([1, 4], [0.5, 0.5], [0, 1], ["00", "11"])
    model = hb.HlaAttrBagObj(0, 5, ["a", "b"], [c1, c2])
    G = np.array([[0, 0, 0, 0, 0], [2, 2, 2, 2, 2], [0, 1, 0, 1, 1], [1, 1, 1, 1, 1], [NA] * 5, [0, NA, 2, 1, NA]], np.int32)
    return model, G


def underflow_case():
    """A classifier whose every pair is >= 65 mismatches away has total 0, so 1/total = inf and 0 * inf = NaN poisons the
    whole sample (src/LibHLA.cpp:1826-1828)."""
    k = 100
    far = hb.Classifier(np.arange(k), [0.5, 0.5], [0, 1], ["1" * k, "1" * k])
    near = hb.Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    model = hb.HlaAttrBagObj(0, k, ["a", "b", "c"], [near, far])
    G = np.zeros((3, k), np.int32)
    G[1, 40:] = NA
    G[2, :] = NA
    return model, G


def test_two_alleles_three_cells():
    model, G = two_allele_case()
    parts = np.array([[0, 1], [0, 0], [1, 0]], np.int32)
    for vote, (got, _) in run_case(model, G, parts, what="2 alleles").items():
        assert model.n_cell == 3 and (got["g1"][:, 0] != NA).any() and (got["g1"][:, 0] == NA).any(), vote
        # the partition with the ids swapped: the same bins under other names
        assert np.array_equal(got["prob"][:, 0], got["prob"][:, 2], equal_nan=True)
        assert np.array_equal(got["dosage"][:, 0:2], got["dosage"][:, 3:5][:, ::-1], equal_nan=True)


def test_nan_posteriors_and_an_empty_group():
    model, G = underflow_case()
    parts = np.array([[0, 1, 2], [0, 0, 1], [0, 0, 0], [2, 0, 0]], np.int32)        # (the last one: group 1 has no allele)
    res = run_case(model, G, parts, what="underflow")
    got, want = res[1]
    assert np.isnan(want["postprob"][0]).all() and want["call"]["h1"][0] == NA            # the corner is there
    assert np.all(got["g1"][0] == NA) and np.all(got["prob"][0] == 0.0)                   # a NaN bin never wins; no weight sum is NaN
    assert np.all(got["g1"][2] == NA) and np.all(got["prob"][2] == 0.0)                   # all missing
    off = np.concatenate([[0], np.cumsum(levels_of(parts))])
    assert np.all(got["dosage"][:, off[3] + 1] == 0.0)                                    # the empty group


# 7 ---------------------------------------------------------------------------------------------------------------
def test_cohort_larger_than_a_batch_host_entry_and_device_entry():
    """More samples than batch_limit(): the host entry goes through the three-stream slices, the device entry through
    several batches of one resident matrix; both equal the reference computed in one piece."""
    import torch
    model, founders, af = synth.make_model("hla-a-small")
    h = np.arange(model.n_hla)
    parts = np.stack([h % 3, h, h // 4]).astype(np.int32)
    dev = hb.hlaModelFromObj(model)
    try:
        ns = dev.batch_limit() + 3017
        G, _ = synth.make_samples(founders, af, ns, seed=31)
        G[ns - 1, :] = NA
        want = groups(model, G, parts)
        with dev.groups_plan(parts) as plan:
            got = dev.predict_groups(G, plan, 1)
            assert dev.status() == 0 and dev.handover_faults() == 0
            assert_groups_equal(got, want, "host entry")
            tdev = torch.device("cuda", dev.device())
            dg = torch.from_numpy(G).to(tdev)
            q, d = plan.n_part, plan.n_level
            o = dict(g1=torch.empty((ns, q), dtype=torch.int32, device=tdev), g2=torch.empty((ns, q), dtype=torch.int32, device=tdev),
                     prob=torch.empty((ns, q), dtype=torch.float64, device=tdev), matching=torch.empty(ns, dtype=torch.float64, device=tdev),
                     dosage=torch.empty((ns, d), dtype=torch.float64, device=tdev))
            torch.cuda.synchronize(tdev)
            st = torch.cuda.current_stream(tdev)
            dev.predict_groups_device(dg.data_ptr(), ns, plan, o["g1"].data_ptr(), o["g2"].data_ptr(), o["prob"].data_ptr(),
                                      o["matching"].data_ptr(), o["dosage"].data_ptr(), vote_method=1, stream=st.cuda_stream)
            st.synchronize()
            assert dev.status() == 0
            assert_groups_equal({key: o[key].cpu().numpy() for key in o}, want, "device entry")
    finally:
        dev.close()


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def benchmark_batch():
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 10_000)
    parts = random_partitions(model.n_hla, [3, 6], seed=17)
    return model, G, parts, groups(model, G, parts)


@pytest.mark.parametrize("which_pass", [1, 2])
def test_host_entry_repairs_a_dropped_handover(which_pass, benchmark_batch):
    """The benchmark batch (both passes have cut tails): with the first hand-over of a pass dropped the poisoned calls are
    never returned -- the library runs the call again without hand-overs.  (Two samples of this batch hold NaN in their
    posterior by an underflow, one of them in all cells but one: a bin with a NaN cell never wins, the others may.)"""
    model, G, parts, want = benchmark_batch
    m = hb.hlaModelFromObj(model)
    try:
        with m.groups_plan(parts) as plan:
            m.inject_handover_fault(which_pass)
            got = m.predict_groups(G, plan, 1)
            assert m.handover_faults() == 1 and m.status() == 0
    finally:
        m.close()
    assert np.isnan(want["postprob"]).any(axis=1).sum() == 2          # (a change of the synthetic batch is to be noticed)
    assert not np.isnan(got["prob"]).any()
    assert_groups_equal(got, want, f"repair, pass {which_pass}")


# 9 ---------------------------------------------------------------------------------------------------------------
def toy_alignment(alleles, seed=1, length=8):
    """A made-up alignment: position 3 and 6 the same letter everywhere; one allele without a sequence."""
    rng = np.random.default_rng(seed)
    seq = {}
    for i, a in enumerate(alleles):
        s = [str(rng.choice(list("ARN"))) for _ in range(length)]
        s[2] = s[5] = "M"
        if i != 4:
            seq[a] = "".join(s)
    return seq


def _assert_groups_are(r, res, grp, what, want_dosage=True):
    """The reference applied to hlaPredict(type="response+prob")'s matrix [n_cell, n_samp]."""
    want = groups_from_postprob(np.ascontiguousarray(res.postprob.T), len(grp.alleles), grp.group_of)
    want["matching"] = res.matching
    assert_groups_equal({"g1": r.g1, "g2": r.g2, "prob": r.prob, "matching": r.matching, "dosage": r.dosage}, want, what)
    assert (r.dosage is not None) == want_dosage
    assert r.sample_id == list(res.sample_id) and r.assembly == res.assembly and r.locus == res.locus and r.groups is grp
    assert r.offsets.tolist() == grp.offsets.tolist()


def mapped_cohort(model, G):
    """An hlaSNPGenoClass whose SNPs are a reordered subset of the model's, a third of them with reversed alleles, plus
    SNPs the model does not know (the recipe of tests/test_hip_draws.py)."""
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
    return hb.HlaSNPGeno(genotype=np.array([rows[i] for i in order], np.int32), sample_id=[f"s{i}" for i in range(n_samp)],
                         snp_id=[ids[i] for i in order], snp_position=np.array([pos[i] for i in order], np.float64),
                         snp_allele=[alle[i] for i in order], assembly="hg19")


@pytest.mark.parametrize("vote", ["prob", "majority"])
def test_hla_predict_groups_end_to_end(vote, model_a):
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 333, seed=12, miss=0.3)
    G[5, :] = NA
    grp = (hb.hlaGroupsByResolution(model.hla_allele, "2-digit") + hb.hlaGroupsByMap(model.hla_allele, {"01:01": "x", "03:02": "x"}, "x")
           + hb.hlaGroupsBySequence(model.hla_allele, toy_alignment(model.hla_allele)))
    assert "3" not in grp.names and "6" not in grp.names and any("?" in lv for lv in grp.levels)
    m = hb.hlaModelFromObj(model)
    try:
        snp = mapped_cohort(model, G)
        for order in ("C", "F"):
            snp.genotype = np.asarray(snp.genotype, order=order)
            with pytest.warns(UserWarning, match="No prediction output"):
                r = hb.hlaPredictGroups(m, snp, grp, vote=vote, verbose=False)
            with pytest.warns(UserWarning):
                res = hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False)
            _assert_groups_are(r, res, grp, f"HlaSNPGeno {order}")
        # calls(q) and dosage_of(q) carry the level names
        q = grp.index("2-digit")
        one = r.calls("2-digit")
        lv = grp.levels[q]
        assert one.allele1 == [None if g == NA else lv[g] for g in r.g1[:, q]]
        assert one.allele2 == [None if g == NA else lv[g] for g in r.g2[:, q]]
        assert np.array_equal(one.prob, r.prob[:, q]) and one.allele1[5] is None
        assert r.dosage_of(q).shape == (len(lv), 333) and np.array_equal(r.dosage_of(q), one.dosage)
        assert np.array_equal(r.dosage_of(q), r.dosage[:, grp.offsets[q]:grp.offsets[q + 1]].T)
        with hb.HlaDeviceCohort(snp) as coh:
            with pytest.warns(UserWarning, match="No prediction output"):
                rc = hb.hlaPredictGroups(m, coh, grp, vote=vote, verbose=False)
        _assert_groups_are(rc, res, grp, "HlaDeviceCohort")
        for mat, what in ((np.ascontiguousarray(G[:100].T), "C"), (np.asfortranarray(G[:100].T), "F"),
                          (np.ascontiguousarray(G[:100].T).astype(np.float64), "float"), (G[3].copy(), "vector")):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = hb.hlaPredictGroups(m, mat, grp, dosage=(what != "F"), vote=vote, verbose=False)
                res = hb.hlaPredict(m, mat, type="response+prob", vote=vote, verbose=False)
            _assert_groups_are(r, res, grp, what, want_dosage=(what != "F"))
        # a raw integer matrix is taken as it is
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            raw = hb.hlaPredictGroups(m, mat, grp.group_of[:2], vote=vote, verbose=False)
        assert np.array_equal(raw.g1, r.g1[:, :2]) and np.array_equal(raw.prob, r.prob[:, :2], equal_nan=True)
        assert raw.groups.levels[0] == [str(i) for i in range(len(grp.levels[0]))]
    finally:
        m.close()
    # the lazily opened BED file of the HapMap fixture
    lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
    grp_a = hb.hlaGroupsByResolution(model_a.hla_allele, "2-digit") + hb.HlaAlleleGroups.from_matrix(model_a.hla_allele, identity(model_a.n_hla))
    m = hb.hlaModelFromObj(model_a)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictGroups(m, lazy, grp_a, vote=vote, match_type="RefSNP", verbose=False)
            res = hb.hlaPredict(m, lazy, type="response+prob", vote=vote, match_type="RefSNP", verbose=False)
        _assert_groups_are(r, res, grp_a, "BED")
        assert np.array_equal(r.g1[:, 1], res.h1) and np.array_equal(r.g2[:, 1], res.h2)
        assert np.array_equal(r.prob[:, 1], res.prob, equal_nan=True) and np.array_equal(r.dosage_of(1), res.dosage, equal_nan=True)
    finally:
        m.close()


def test_verbose_text(model_a, hapmap_geno, capsys):
    m = hb.hlaModelFromObj(model_a)
    grp = hb.hlaGroupsByResolution(model_a.hla_allele, "2-digit")
    try:
        hb.hlaPredictGroups(m, hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(5))), grp, match_type="RefSNP")
    finally:
        m.close()
    text = capsys.readouterr().out
    assert f"1 partition of the alleles ({grp.n_level} groups" in text and "# of samples: 5" in text


# 10 --------------------------------------------------------------------------------------------------------------
def test_two_digit_calls_agree_with_the_merge_of_one_model(hla_b_case):
    """hlaPredictMerge([model], max_resolution="2-digit") collapses the same posterior to the two-digit names and
    renormalises.  Both sum the same at most n_cell non-negative terms in FP64 and differ by the order and by one division
    by a sum within n_cell * 2^-53 of 1: the probabilities agree within n_cell * 2^-52 < 3e-13 (1,275 cells), asserted
    at 1e-12 relative; the called names are the same wherever the two largest bins differ by more than that."""
    model, G, _ = hla_b_case
    grp = hb.hlaGroupsByResolution(model.hla_allele, "2-digit")
    snp = synth.as_snp_geno(model, G)
    m = hb.hlaModelFromObj(model)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictGroups(m, snp, grp, verbose=False)
            mg = hb.hlaPredictMerge([m], snp, max_resolution="2-digit", use_matching=False, ret_postprob=True, verbose=False)
    finally:
        m.close()
    ok = r.g1[:, 0] != NA
    assert ok.sum() >= 290 and not ok[0]
    mine = r.calls(0)
    post = np.asarray(mg.postprob)[:, ok]                              # [merged pairs, samples]
    top2 = np.sort(post, axis=0)[-2:]
    clear = (top2[1] - top2[0]) > 1e-12 * top2[1]
    rel = np.abs(r.prob[ok, 0] - np.asarray(mg.prob)[ok]) / r.prob[ok, 0]
    print("largest relative difference of the probabilities:", float(rel.max()), "clear calls:", int(clear.sum()), "of", int(ok.sum()))
    assert np.all(rel <= 1e-12)
    a = [tuple(sorted((mine.allele1[i], mine.allele2[i]))) for i in np.where(ok)[0]]
    b = [tuple(sorted((mg.allele1[i], mg.allele2[i]))) for i in np.where(ok)[0]]
    assert all(x == y for x, y, c in zip(a, b, clear) if c) and clear.sum() >= 250


# 11 --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_call(model_a, model_oob, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    ns, n = len(G), model_a.n_hla
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: L.hibag_hip_last_error().decode()
    parts = np.concatenate([identity(n), (np.arange(n) % 2)[None, :].astype(np.int32)])
    Q, D = 2, n + 2
    g1, g2 = np.empty((ns, Q), np.int32), np.empty((ns, Q), np.int32)
    pr, mt, ds = np.empty((ns, Q)), np.empty(ns), np.empty((ns, D))
    col = np.arange(model_a.n_snp, dtype=np.int32)
    dev = hb.hlaModelFromObj(model_a)
    other = hb.hlaModelFromObj(model_oob)
    try:
        # plan creation
        def create(model, q, mat):
            h = C.c_void_p()
            rc = L.hibag_hip_groups_create(model.handle, q, p(mat), C.byref(h))
            assert (rc == 0) == bool(h.value)
            return rc, h
        big = np.zeros((GROUPS_MAX_PART + 1, n), np.int32)
        assert create(dev, 0, big)[0] == -1 and "HIBAG_HIP_GROUPS_MAX_PART" in err()
        assert create(dev, GROUPS_MAX_PART + 1, big)[0] == -1 and str(GROUPS_MAX_PART) in err()
        many = np.tile(identity(n), (GROUPS_MAX_LEVELS // n + 1, 1))            # D just above the limit
        assert len(many) <= GROUPS_MAX_PART and create(dev, len(many), many)[0] == -1 and "HIBAG_HIP_GROUPS_MAX_LEVELS" in err()
        for bad_id in (n, -1):
            bad = parts.copy()
            bad[1, 3] = bad_id
            assert create(dev, 2, bad)[0] == -1 and "group_of[1][3]" in err(), bad_id
        assert create(dev, 2, None)[0] == -1
        assert L.hibag_hip_groups_create(None, 2, p(parts), C.byref(C.c_void_p())) == -1
        rc, plan = create(dev, 2, parts)
        assert rc == 0
        rc, foreign = create(other, 1, identity(model_oob.n_hla))
        assert rc == 0
        lv = np.empty(2, np.int32)
        assert L.hibag_hip_groups_levels(plan, p(lv)) == 0 and lv.tolist() == [n, 2]
        assert L.hibag_hip_groups_levels(None, p(lv)) == -1 and L.hibag_hip_groups_tile(None, None) == -1

        call = lambda pl, a, b, c, d, e, n_samp=ns, vote=1: L.hibag_hip_predict_groups(
            dev.handle, p(G), n_samp, vote, pl, p(a), p(b), p(c), p(d), p(e))
        entries = {
            "host": lambda pl: call(pl, g1, g2, pr, mt, ds),
            "device": lambda pl: L.hibag_hip_predict_groups_device(dev.handle, p(G), ns, 1, pl, p(g1), p(g2), p(pr), p(mt), p(ds), None),
            "mapped": lambda pl: L.hibag_hip_predict_groups_mapped(dev.handle, p(G), ns, G.shape[1], p(col), None, 1, pl,
                                                                   p(g1), p(g2), p(pr), p(mt), p(ds)),
            "snp_major": lambda pl: L.hibag_hip_predict_groups_snp_major(dev.handle, p(G), ns, ns, G.shape[1], None, None, 1, pl,
                                                                         p(g1), p(g2), p(pr), p(mt), p(ds)),
            "bed": lambda pl: L.hibag_hip_predict_groups_bed(dev.handle, BED.encode(), 90, 5316, p(col), None, 1, pl,
                                                             p(g1), p(g2), p(pr), p(mt), p(ds)),
        }
        snp = synth.as_snp_geno(model_a, G)
        with hb.HlaDeviceCohort(snp) as coh:
            entries["cohort"] = lambda pl: L.hibag_hip_predict_groups_cohort(dev.handle, coh.handle, 0, ns, p(col), None, 1, pl,
                                                                             p(g1), p(g2), p(pr), p(mt), p(ds))
            for name, f in entries.items():
                assert f(None) == -1 and "plan" in err(), name
                assert f(foreign) == -1 and "another model" in err(), name
        for args in ((None, g2, pr, mt, ds), (g1, None, pr, mt, ds), (g1, g2, None, mt, ds)):
            assert call(plan, *args) == -1 and "required" in err()
        assert call(plan, g1, g2, pr, mt, ds, n_samp=-1) == -1
        assert call(plan, g1, g2, pr, mt, ds, vote=3) == -1 and "vote_method" in err()
        assert dev.status() == 0
        # the model is still usable; matching and dosage may be NULL
        assert call(plan, g1, g2, pr, None, None) == 0
        want = groups(model_a, G, parts)
        assert_groups_equal({"g1": g1, "g2": g2, "prob": pr}, want, "after the rejected calls", keys=("g1", "g2", "prob"))
        assert call(plan, g1, g2, pr, mt, ds) == 0
        assert_groups_equal({"g1": g1, "g2": g2, "prob": pr, "matching": mt, "dosage": ds}, want, "after the rejected calls")
        assert call(plan, None, None, None, None, None, n_samp=0) == 0                   # nothing to write
        assert dev.status() == 0
        L.hibag_hip_groups_free(plan)
        L.hibag_hip_groups_free(foreign)
        L.hibag_hip_groups_free(None)
        # the Python layer says the same in its own words
        with pytest.raises(ValueError):
            dev.groups_plan(np.zeros((1, n + 1), np.int32))
        with pytest.raises(hb.HibagHipError):
            dev.groups_plan(np.full((1, n), n, np.int32))
        with pytest.raises(ValueError):
            hb.hlaPredictGroups(dev, G.T, hb.hlaGroupsByResolution(list(model_a.hla_allele)[:-1]), verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictGroups(dev, G.T, np.tile(identity(n), (GROUPS_MAX_LEVELS // n + 1, 1)), verbose=False)
    finally:
        dev.close()
        other.close()
