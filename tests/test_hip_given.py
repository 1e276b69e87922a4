"""hlaPredictGiven on the GPU: hibag_hip_predict_given and its routes equal, every sample and both vote methods, to the
reference (tests/given_reference.py: the contract of DESIGN.md section 18 applied to the CPU oracle's posterior matrix); full
sets are predict_raw's own call, probability and dosage; independent of batches, slices, routes, a repaired hand-over and of
whether dosages were asked for; the model's other outputs untouched; invalid arguments rejected.  Every comparison is exact
equality (NaN == NaN)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import hibag_amd as hb
from conftest import REFDATA, align_geno
from given_reference import assert_given_equal, conditional, full_sets, given, given_from_postprob, pack
from hibag_amd import NA_INTEGER, _lib, synth

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")
OUT = ("h1", "h2", "prob", "support", "matching")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def random_sets(n_samp, n_hla, seed):
    """Every allele in A and in B with probability 0.5; sample 0 has A empty, sample 1 has B empty, sample 2 both full."""
    allowed = np.random.default_rng(seed).random((n_samp, 2, n_hla)) < 0.5
    if n_samp > 0:
        allowed[0, 0] = False
    if n_samp > 1:
        allowed[1, 1] = False
    if n_samp > 2:
        allowed[2] = True
    return allowed


def cut(ref, idx):
    """Samples `idx` (a slice or an index array) of a reference."""
    return {k: ref[k][idx] for k in OUT + ("dosage",) if k in ref}


def check_shape(got, n_samp, n_hla, want_dosage):
    for key in ("h1", "h2"):
        assert got[key].shape == (n_samp,) and got[key].dtype == np.int32, key
    for key in ("prob", "support", "matching"):
        assert got[key].shape == (n_samp,) and got[key].dtype == np.float64, key
    assert ("dosage" in got) == want_dosage
    if want_dosage:
        assert got["dosage"].shape == (n_samp, n_hla)
    na = got["h1"] == NA
    assert np.array_equal(na, got["h2"] == NA) and np.all(got["h1"][~na] <= got["h2"][~na]) and np.all(got["h1"][~na] >= 0)


def run_case(model, G, allowed, votes=(1, 2), what="", refs=None):
    """predict_given, with and without dosages, against the reference; returns {vote: (got, want, raw)}."""
    out = {}
    packed = pack(allowed)
    dev = hb.hlaModelFromObj(model)
    try:
        for vote in votes:
            got = dev.predict_given(G, packed, vote, want_dosage=True)
            lean = dev.predict_given(G, packed, vote, want_dosage=False)
            raw = dev.predict_raw(G, vote, want_dosage=True)
            assert dev.status() == 0 and dev.handover_faults() == 0
            want = refs[vote] if refs is not None else given(model, G, allowed, vote=vote)
            check_shape(got, len(G), model.n_hla, True)
            check_shape(lean, len(G), model.n_hla, False)
            assert_given_equal(got, want, f"{what} vote={vote}")
            for key in OUT:                                   # the optional output changes nothing
                assert np.array_equal(got[key], lean[key], equal_nan=True), (what, vote, key)
            assert np.array_equal(got["matching"], raw["matching"], equal_nan=True), (what, vote)
            out[vote] = (got, want, raw)
    finally:
        dev.close()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------
# A mask word holds 32 alleles: n_hla = 2 (one word, three cells), 31 / 32 / 33 (a word just not / exactly / not any more
# enough), 64 / 65 (the same at the second boundary).
@pytest.mark.parametrize("n", [2, 31, 32, 33, 64, 65])
def test_mask_word_boundaries(n):
    model, founders, af = synth.make_model("hla-a-small", seed=11, n_hla=n, n_haplo=max(40, 2 * n), n_classifier=6)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.85)
    G[77, :] = NA
    allowed = random_sets(130, n, seed=100 + n)
    res = run_case(model, G, allowed, what=f"n_hla={n}")
    for vote, (got, want, raw) in res.items():
        assert got["h1"][0] == NA and got["h1"][1] == NA and got["support"][0] == 0.0 and got["support"][1] == 0.0, vote
        assert got["h1"][77] == NA and got["prob"][77] == 0.0 and got["support"][77] == 0.0 and np.isnan(got["matching"][77]), vote
        for key in ("h1", "h2", "prob", "dosage"):            # sample 2: both sets full
            assert np.array_equal(got[key][2], raw[key][2], equal_nan=True), (vote, key)
    # the corner is present: the constraint changes calls, and calls reach into the last mask word
    got, _, raw = res[1]
    differ = int(np.count_nonzero((got["h1"] != raw["h1"]) | (got["h2"] != raw["h2"])))
    last = int(np.count_nonzero((got["h1"] != NA) & (got["h2"] >= 32 * ((n - 1) // 32))))
    print(f"n_hla={n}: {differ} of 130 calls differ from predict_raw's, {int((got['h1'] == NA).sum())} NA, "
          f"{last} called pairs hold an allele of the last mask word")
    assert differ >= 1
    if n in (33, 65):
        assert last >= 1


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread_case():
    """tests/test_given_host.py's corner: 14 alleles, 105 cells, 85 % of the genotypes missing, 130 samples, sample 77 with
    every SNP missing; the reference is made once per vote."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.85)
    G[77, :] = NA
    allowed = random_sets(130, model.n_hla, seed=7)
    refs = {vote: given(model, G, allowed, vote=vote) for vote in (1, 2)}
    return model, G, allowed, refs


# lane = sample, a wavefront is 64 of them: one sample, a wavefront just not / exactly / not any more full, three wavefronts
@pytest.mark.parametrize("n_samp", [1, 63, 64, 65, 130])
def test_lane_mapping(n_samp, spread_case):
    model, G, allowed, refs = spread_case
    # the LAST n_samp samples: every sample sits in another lane than in the full batch, the other samples' sets are gone
    sl = slice(130 - n_samp, 130)
    want = {vote: cut(refs[vote], sl) for vote in (1, 2)}
    run_case(model, np.ascontiguousarray(G[sl]), allowed[sl], what=f"n_samp={n_samp}", refs=want)


# 3 ---------------------------------------------------------------------------------------------------------------
def assert_rule_6(model, G, what):
    """Full sets on the device against predict_raw itself, and predict_raw identical before and after."""
    ns, n = len(G), model.n_hla
    packed = pack(full_sets(ns, n))
    dev = hb.hlaModelFromObj(model)
    try:
        before = {vote: dev.predict_raw(G, vote, want_dosage=True, want_prob=True) for vote in (1, 2)}
        for vote in (1, 2):
            got = dev.predict_given(G, packed, vote, want_dosage=True)
            raw = before[vote]
            for key in ("h1", "h2", "prob", "dosage", "matching"):
                assert np.array_equal(got[key], raw[key], equal_nan=True), (what, vote, key)
            assert np.array_equal(got["support"], np.cumsum(raw["postprob"], axis=1)[:, -1], equal_nan=True), (what, vote)
        after = {vote: dev.predict_raw(G, vote, want_dosage=True, want_prob=True) for vote in (1, 2)}
        assert dev.status() == 0 and dev.handover_faults() == 0
        return dev.stored_cells(), dev.second_pass_pairs(), before
    finally:
        dev.close()
        for vote in (1, 2):
            for key in before[vote]:
                assert np.array_equal(before[vote][key], after[vote][key], equal_nan=True), (what, vote, key)


def test_full_sets_are_predict_raw_on_the_hla_b_shape():
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 300)
    G[0, :] = NA
    assert model.n_cell == 1275
    _, _, before = assert_rule_6(model, G, "hla-b")
    assert before[1]["h1"][0] == NA and (before[1]["h1"][1:] != NA).sum() >= 290


def test_full_sets_are_predict_raw_on_the_drb1_shape():
    """The large-n_cell, store-every-cell layout (pass 2 = k_accum_cells): 1,830 cells."""
    model, founders, af = synth.make_model("hla-drb1", n_classifier=8)
    G, _ = synth.make_samples(founders, af, 200)
    G[7, :] = NA
    stored, second, _ = assert_rule_6(model, G, "drb1")
    assert stored > 0 and second == 0
    # and a constraint on this layout
    run_case(model, G, random_sets(200, model.n_hla, seed=9), votes=(1,), what="drb1")


# 4 ---------------------------------------------------------------------------------------------------------------
def two_allele_case():
    c1 = hb.Classifier([0, 1, 2, 3], [0.3, 0.3, 0.4], [0, 1, 1], ["0000", "0101", "1111"])
    c2 = hb.Classifier([1, 4], [0.5, 0.5], [0, 1], ["00", "11"])
    model = hb.HlaAttrBagObj(0, 5, ["a", "b"], [c1, c2])
    G = np.array([[0, 0, 0, 0, 0], [2, 2, 2, 2, 2], [0, 1, 0, 1, 1], [1, 1, 1, 1, 1], [NA] * 5, [0, NA, 2, 1, NA]], np.int32)
    return model, G


def underflow_case():
    """A classifier whose every pair is >= 65 mismatches away has total 0, so 1/total = inf and 0 * inf = NaN poisons the
    whole sample (src/LibHLA.cpp:1826-1828): tests/test_hip_groups.py's model."""
    k = 100
    far = hb.Classifier(np.arange(k), [0.5, 0.5], [0, 1], ["1" * k, "1" * k])
    near = hb.Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    model = hb.HlaAttrBagObj(0, k, ["a", "b", "c"], [near, far])
    G = np.zeros((3, k), np.int32)
    G[1, 40:] = NA
    G[2, :] = NA
    return model, G


def all_set_pairs(n_hla):
    """Every pair (A, B) of subsets of n_hla alleles: [4^n_hla, 2, n_hla]."""
    subsets = [[bool((m >> h) & 1) for h in range(n_hla)] for m in range(1 << n_hla)]
    return np.array([[a, b] for a in subsets for b in subsets], np.bool_)


def test_two_alleles_three_cells_under_every_constraint():
    model, G = two_allele_case()
    sets = all_set_pairs(2)                                   # 16 constraints
    assert model.n_cell == 3
    Gs = np.ascontiguousarray(np.repeat(G, len(sets), axis=0))
    allowed = np.ascontiguousarray(np.tile(sets, (len(G), 1, 1)))
    for vote, (got, _, _) in run_case(model, Gs, allowed, what="2 alleles").items():
        assert (got["h1"] != NA).any() and (got["h1"] == NA).any(), vote


def test_nan_posterior_rows_never_win_and_poison_the_support_where_consistent():
    model, G = underflow_case()
    sets = all_set_pairs(3)                                   # 64 constraints
    Gs = np.ascontiguousarray(np.repeat(G, len(sets), axis=0))
    allowed = np.ascontiguousarray(np.tile(sets, (len(G), 1, 1)))
    got, want, _ = run_case(model, Gs, allowed, votes=(1,), what="underflow")[1]
    row0 = slice(0, len(sets))                                # sample 0: every cell NaN
    assert np.isnan(want["postprob"][0]).all() and want["call"]["h1"][0] == NA                 # the corner is there
    assert np.all(got["h1"][row0] == NA) and np.all(got["prob"][row0] == 0.0)                   # never wins; no weight sum is NaN
    A, B = sets[:, 0], sets[:, 1]
    some_cell = A.any(axis=1) & B.any(axis=1)                 # a consistent cell exists iff neither set is empty
    assert np.array_equal(np.isnan(got["support"][row0]), some_cell)
    assert np.all(got["support"][row0][~some_cell] == 0.0)
    last = slice(2 * len(sets), 3 * len(sets))                # sample 2: all missing
    assert np.all(got["h1"][last] == NA) and np.all(got["prob"][last] == 0.0) and np.all(got["support"][last] == 0.0)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_cohort_larger_than_a_batch_host_entry_and_device_entry():
    """More samples than batch_limit(): the host entry goes through the three-stream slices, the device entry through
    several batches of one resident matrix; both equal the reference computed in one piece."""
    import torch
    model, founders, af = synth.make_model("hla-a-small")
    n = model.n_hla
    dev = hb.hlaModelFromObj(model)
    try:
        ns = dev.batch_limit() + 3017
        G, _ = synth.make_samples(founders, af, ns, seed=31)
        G[ns - 1, :] = NA
        allowed = random_sets(ns, n, seed=32)
        packed = pack(allowed)
        want = given(model, G, allowed)
        got = dev.predict_given(G, packed, 1, want_dosage=True)
        assert dev.status() == 0 and dev.handover_faults() == 0
        assert_given_equal(got, want, "host entry")
        tdev = torch.device("cuda", dev.device())
        dg = torch.from_numpy(G).to(tdev)
        da = torch.from_numpy(packed.view(np.int32)).to(tdev)
        f64 = dict(dtype=torch.float64, device=tdev)
        o = dict(h1=torch.empty(ns, dtype=torch.int32, device=tdev), h2=torch.empty(ns, dtype=torch.int32, device=tdev),
                 prob=torch.empty(ns, **f64), support=torch.empty(ns, **f64), matching=torch.empty(ns, **f64),
                 dosage=torch.empty((ns, n), **f64))
        torch.cuda.synchronize(tdev)
        st = torch.cuda.current_stream(tdev)
        dev.predict_given_device(dg.data_ptr(), ns, da.data_ptr(), o["h1"].data_ptr(), o["h2"].data_ptr(), o["prob"].data_ptr(),
                                 o["support"].data_ptr(), o["matching"].data_ptr(), o["dosage"].data_ptr(), vote_method=1,
                                 stream=st.cuda_stream)
        st.synchronize()
        assert dev.status() == 0
        assert_given_equal({key: o[key].cpu().numpy() for key in o}, want, "device entry")
    finally:
        dev.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def benchmark_batch():
    model, founders, af = synth.make_model("hla-b")
    G, truth = synth.make_samples(founders, af, 10_000)
    two_digit = np.arange(model.n_hla) // 4                   # the synthetic names' first field
    allowed = np.stack([two_digit[None, :] == two_digit[truth[:, j]][:, None] for j in (0, 1)], axis=1)
    return model, G, allowed, given(model, G, allowed)


@pytest.mark.parametrize("which_pass", [1, 2])
def test_host_entry_repairs_a_dropped_handover(which_pass, benchmark_batch):
    """The benchmark batch (both passes have cut tails): with the first hand-over of a pass dropped the poisoned calls are
    never returned -- the library runs the call again without hand-overs, the constraint with it."""
    model, G, allowed, want = benchmark_batch
    m = hb.hlaModelFromObj(model)
    try:
        m.inject_handover_fault(which_pass)
        got = m.predict_given(G, pack(allowed), 1, want_dosage=True)
        assert m.handover_faults() == 1 and m.status() == 0
    finally:
        m.close()
    assert_given_equal(got, want, f"repair, pass {which_pass}")


# 7 ---------------------------------------------------------------------------------------------------------------
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


def _assert_given_is(r, res, allowed, what, want_dosage):
    """The reference applied to hlaPredict(type="response+prob")'s matrix [n_cell, n_samp], then rule 5."""
    n_hla = len(r.alleles)
    want = given_from_postprob(np.ascontiguousarray(res.postprob.T), n_hla, allowed)
    want["matching"] = res.matching
    got = {"h1": r.h1, "h2": r.h2, "prob": r.prob_joint, "support": r.support, "matching": r.matching}
    assert_given_equal(got, want, what, keys=OUT)
    cond = conditional(want)
    assert np.array_equal(r.prob, cond["prob"], equal_nan=True), what
    assert (r.dosage is not None) == want_dosage
    if want_dosage:
        assert r.dosage.shape == (n_hla, len(r.sample_id)) and np.array_equal(r.dosage, cond["dosage"].T, equal_nan=True), what
    assert r.sample_id == list(res.sample_id) and r.assembly == res.assembly and r.locus == res.locus
    assert np.array_equal(r.constraint.allowed, allowed)
    calls = r.calls()
    assert calls.allele1 == [None if h == NA else r.alleles[h] for h in r.h1] and calls.prob is r.prob


@pytest.mark.parametrize("vote", ["prob", "majority"])
def test_hla_predict_given_end_to_end(vote, model_a, hla_type_table):
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, truth = synth.make_samples(founders, af, 333, seed=12, miss=0.3)
    G[5, :] = NA
    names = list(model.hla_allele)
    # what is known: the two-digit type of both alleles, of one, of none; sample ids reordered, every seventh sample absent
    a1 = [hb.hlaAlleleDigit([names[t]], "2-digit")[0] for t in truth[:, 0]]
    a2 = [hb.hlaAlleleDigit([names[t]], "2-digit")[0] if i % 3 else None for i, t in enumerate(truth[:, 1])]
    have = [i for i in np.random.default_rng(3).permutation(333) if i % 7]
    typed = hb.HlaAlleleClass(locus="A", sample_id=[f"s{i}" for i in have], allele1=[a1[i] for i in have], allele2=[a2[i] for i in have])
    known = hb.hlaConstraintFromAllele(model, typed)
    assert known.n_unmatched == 0 and known.sample_id[0] != "s0"
    allowed = known.rows_for([f"s{i}" for i in range(333)]).allowed
    assert allowed[0].all() and allowed[7].all() and not allowed[1].all() and allowed[3, 1].all() and not allowed[3, 0].all()
    m = hb.hlaModelFromObj(model)
    try:
        snp = mapped_cohort(model, G)
        for order in ("C", "F"):
            snp.genotype = np.asarray(snp.genotype, order=order)
            with pytest.warns(UserWarning, match="No prediction output"):
                r = hb.hlaPredictGiven(m, snp, known, dosage=True, vote=vote, verbose=False)
            with pytest.warns(UserWarning):
                res = hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False)
            _assert_given_is(r, res, allowed, f"HlaSNPGeno {order}", True)
        assert r.h1[5] == NA and r.calls().allele1[5] is None
        with hb.HlaDeviceCohort(snp) as coh:
            with pytest.warns(UserWarning, match="No prediction output"):
                rc = hb.hlaPredictGiven(m, coh, known, vote=vote, verbose=False)
        _assert_given_is(rc, res, allowed, "HlaDeviceCohort", False)
        # matrices and a vector carry no sample ids: the rows are taken in order, in any of the accepted forms
        first = allowed[:100]
        forms = {"C": first, "F": pack(first), "float": hb.HlaAlleleConstraint(names, first), "vector": first[3:4]}
        for mat, what in ((np.ascontiguousarray(G[:100].T), "C"), (np.asfortranarray(G[:100].T), "F"),
                          (np.ascontiguousarray(G[:100].T).astype(np.float64), "float"), (G[3].copy(), "vector")):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = hb.hlaPredictGiven(m, mat, forms[what], dosage=(what != "F"), vote=vote, verbose=False)
                res = hb.hlaPredict(m, mat, type="response+prob", vote=vote, verbose=False)
            _assert_given_is(r, res, first[3:4] if what == "vector" else first, what, what != "F")
    finally:
        m.close()
    # the lazily opened BED file of the HapMap fixture, the HapMap HLA-A types cut to two digits
    lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
    ids = list(hla_type_table["sample.id"])
    cut2 = lambda col: hb.hlaAlleleDigit(list(hla_type_table[col]), "2-digit")
    typed = hb.HlaAlleleClass(locus="A", sample_id=ids, allele1=cut2("A.1"), allele2=cut2("A.2"))
    known = hb.hlaConstraintFromAllele(model_a, typed)
    allowed = known.rows_for(list(lazy.sample_id)).allowed
    assert (~allowed.all(axis=2)).any()
    m = hb.hlaModelFromObj(model_a)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictGiven(m, lazy, known, dosage=True, vote=vote, match_type="RefSNP", verbose=False)
            res = hb.hlaPredict(m, lazy, type="response+prob", vote=vote, match_type="RefSNP", verbose=False)
        _assert_given_is(r, res, allowed, "BED", True)
        # every call made is consistent with the two-digit types
        ok = r.h1 != NA
        two = hb.hlaAlleleDigit(list(model_a.hla_allele), "2-digit")
        i = np.where(ok)[0]
        assert np.all((allowed[i, 0, r.h1[i]] & allowed[i, 1, r.h2[i]]) | (allowed[i, 1, r.h1[i]] & allowed[i, 0, r.h2[i]]))
        assert len(two) == model_a.n_hla
    finally:
        m.close()


def test_verbose_text(model_a, hapmap_geno, capsys):
    m = hb.hlaModelFromObj(model_a)
    n = model_a.n_hla
    allowed = full_sets(5, n)
    allowed[0, 0, 1:] = False
    allowed[1, :, 2:] = False
    try:
        hb.hlaPredictGiven(m, hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(5))), allowed, match_type="RefSNP")
    finally:
        m.close()
    text = capsys.readouterr().out
    assert "consistent with the known partial typing" in text and "# of samples: 5" in text
    assert "1 samples constrained on two chromosomes, 1 on one, 3 on none; 0 unmatched names" in text


# 8 ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_call(model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    ns, n = len(G), model_a.n_hla
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: L.hibag_hip_last_error().decode()
    allowed = random_sets(ns, n, seed=4)
    al = pack(allowed)
    h1, h2 = np.empty(ns, np.int32), np.empty(ns, np.int32)
    pr, sp, mt, ds = np.empty(ns), np.empty(ns), np.empty(ns), np.empty((ns, n))
    col = np.arange(model_a.n_snp, dtype=np.int32)
    dev = hb.hlaModelFromObj(model_a)
    try:
        def entries(m, a, o1, o2, o3, o4, vote=1, coh=None):
            e = {
                "host": lambda: L.hibag_hip_predict_given(m, p(G), ns, vote, p(a), p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
                "device": lambda: L.hibag_hip_predict_given_device(m, p(G), ns, vote, p(a), p(o1), p(o2), p(o3), p(o4), p(mt), p(ds), None),
                "mapped": lambda: L.hibag_hip_predict_given_mapped(m, p(G), ns, G.shape[1], p(col), None, vote, p(a),
                                                                   p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
                "snp_major": lambda: L.hibag_hip_predict_given_snp_major(m, p(G), ns, ns, G.shape[1], None, None, vote, p(a),
                                                                         p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
                "bed": lambda: L.hibag_hip_predict_given_bed(m, BED.encode(), 90, 5316, p(col), None, vote, p(a),
                                                             p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
            }
            if coh is not None:
                e["cohort"] = lambda: L.hibag_hip_predict_given_cohort(m, coh.handle, 0, ns, p(col), None, vote, p(a),
                                                                       p(o1), p(o2), p(o3), p(o4), p(mt), p(ds))
            return e

        # an unfinalized model
        fresh = C.c_void_p(L.hibag_hip_model_new(n, model_a.n_snp))
        assert fresh.value
        snp = synth.as_snp_geno(model_a, G)
        with hb.HlaDeviceCohort(snp) as coh:
            for name, f in entries(fresh, al, h1, h2, pr, sp, coh=coh).items():
                assert f() == -1 and "not finalized" in err(), name
            for name, f in entries(dev.handle, None, h1, h2, pr, sp, coh=coh).items():
                assert f() == -1 and "allow" in err(), name
            for missing in range(4):
                outs = [h1, h2, pr, sp]
                outs[missing] = None
                for name, f in entries(dev.handle, al, *outs, coh=coh).items():
                    assert f() == -1 and "required" in err(), (name, missing)
            for name, f in entries(dev.handle, al, h1, h2, pr, sp, vote=3, coh=coh).items():
                assert f() == -1 and "vote_method" in err(), name
        L.hibag_hip_model_free(fresh)
        assert L.hibag_hip_predict_given(None, p(G), ns, 1, p(al), p(h1), p(h2), p(pr), p(sp), None, None) == -1
        assert L.hibag_hip_predict_given(dev.handle, p(G), -1, 1, p(al), p(h1), p(h2), p(pr), p(sp), None, None) == -1
        assert dev.status() == 0
        # the model is still usable; matching and dosage may be NULL; n_samp == 0 with NULL pointers is fine
        call = lambda a, b: L.hibag_hip_predict_given(dev.handle, p(G), ns, 1, p(al), p(h1), p(h2), p(pr), p(sp), p(a), p(b))
        want = given(model_a, G, allowed)
        assert call(None, None) == 0
        assert_given_equal({"h1": h1, "h2": h2, "prob": pr, "support": sp}, want, "after the rejected calls", keys=("h1", "h2", "prob", "support"))
        assert call(mt, ds) == 0
        assert_given_equal({"h1": h1, "h2": h2, "prob": pr, "support": sp, "matching": mt, "dosage": ds}, want, "after the rejected calls")
        assert L.hibag_hip_predict_given(dev.handle, None, 0, 1, None, None, None, None, None, None, None) == 0
        assert L.hibag_hip_predict_given_device(dev.handle, None, 0, 1, None, None, None, None, None, None, None, None) == 0
        assert dev.status() == 0
        # the Python layer says the same in its own words
        with pytest.raises(ValueError):
            dev.predict_given(G, al[:, :, :0])                             # the wrong word count
        with pytest.raises(ValueError):
            dev.predict_given(G, al[:5])                                   # fewer rows than samples
        with pytest.raises(ValueError):
            dev.predict_given(G, al.astype(np.int64))
        with pytest.raises(ValueError):
            hb.hlaPredictGiven(dev, G.T, allowed[:5], verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictGiven(dev, G.T, hb.HlaAlleleConstraint(list(model_a.hla_allele)[:-1], allowed[:, :, :-1]), verbose=False)
        with pytest.raises(TypeError):
            hb.hlaPredictGiven(dev, G.T, allowed.astype(np.float64), verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictGiven(dev, G.T, allowed, vote="mean", verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictGiven(dev, G.T, allowed, dosage=True, verbose=False)
        assert_given_equal({"h1": r.h1, "h2": r.h2, "prob": r.prob_joint, "support": r.support, "matching": r.matching}, want,
                           "after the rejected calls", keys=OUT)
    finally:
        dev.close()
