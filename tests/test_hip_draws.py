"""hlaPredictDraws on the GPU: hibag_hip_predict_draw and its routes equal, every sample, every draw and both vote methods,
to the reference (tests/draws_reference.py: the contract of DESIGN.md section 16 applied to the CPU oracle's posterior
matrix); independent of batches, slices, routes, a repaired hand-over and the number of draws; `sample0` acts; the model's
other outputs untouched; invalid arguments rejected.  Every comparison is exact equality (NaN == NaN for probabilities):
there is no tolerance in this feature."""
import ctypes as C
import os

import numpy as np
import pytest

import hibag_amd as hb
from conftest import REFDATA, align_geno
from draws_reference import assert_draws_equal, draws, draws_from_postprob
from hibag_amd import NA_INTEGER, _lib, synth
from hibag_amd._lib import DRAW_MAX

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
SEED = 2024
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def check_draws(got, raw, post=None, what=""):
    """matching is predict_raw's; a sample is NA in every draw or in none, exactly where predict_raw has no call (or the
    posterior holds a NaN); every drawn pair is ordered."""
    assert np.array_equal(got["matching"], raw["matching"], equal_nan=True), what
    na = got["h1"] == NA
    assert np.array_equal(na, got["h2"] == NA) and np.all(na == na[:, :1]), what
    ok = ~na
    assert np.all(got["h1"][ok] <= got["h2"][ok]) and np.all(got["h1"][ok] >= 0) and np.all(got["prob"][ok] > 0), what
    assert np.all((got["prob"][na] == 0) | np.isnan(got["prob"][na])), what
    assert np.all(na[raw["h1"] == NA, 0]), what


def run_case(model, G, n, votes=(1, 2), what="", refs=None, seed=SEED):
    """predict_draw against the reference, both votes; returns {vote: (got, want)}.  `refs` {vote: draws(...) of at least
    n draws}: the oracle is run once for several n (the reference's draws are a prefix of a longer list's)."""
    out = {}
    dev = hb.hlaModelFromObj(model)
    try:
        for vote in votes:
            got = dev.predict_draw(G, n, seed, vote)
            raw = dev.predict_raw(G, vote, want_dosage=False)
            assert dev.status() == 0 and dev.handover_faults() == 0
            if refs is not None:
                want = dict(draws_from_postprob(refs[vote]["postprob"], n, seed, 0, int(model.n_hla)),
                            matching=refs[vote]["matching"], postprob=refs[vote]["postprob"], call=refs[vote]["call"])
            else:
                want = draws(model, G, n, seed, vote=vote)
            assert got["h1"].shape == (len(G), n) and got["h1"].dtype == np.int32 and got["prob"].dtype == np.float64
            assert_draws_equal(got, want, f"{what} n={n} vote={vote}")
            check_draws(got, raw, what=f"{what} n={n} vote={vote}")
            out[vote] = (got, want)
    finally:
        dev.close()
    return out


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_fixture_models_on_the_hapmap_genotypes(which, request, hapmap_geno):
    model = request.getfixturevalue(which)
    G = align_geno(model, hapmap_geno, hapmap_geno.sample_id)
    refs = {vote: draws(model, G, DRAW_MAX, SEED, vote=vote) for vote in (1, 2)}
    for n in (1, 5, DRAW_MAX):
        run_case(model, G, n, what=which, refs=refs)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread_case():
    """14 alleles, 105 cells (not a multiple of 8); half the genotypes missing, so the posteriors are spread over many
    pairs; 130 samples: two full groups and a partial one of 2; one sample with every SNP missing."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.5)
    G[77, :] = NA
    refs = {vote: draws(model, G, DRAW_MAX, SEED, vote=vote) for vote in (1, 2)}
    return model, G, refs


def test_spread_posteriors_the_corner_is_there(spread_case):
    """Without it every test here would pass on an arg-max."""
    model, G, refs = spread_case
    assert model.n_cell == 105
    for vote in (1, 2):
        r = refs[vote]
        ok = r["call"]["h1"] != NA
        assert ok.sum() >= 100 and not ok[77]
        h1, h2 = r["h1"][ok, :16], r["h2"][ok, :16]
        differ = (h1 != r["call"]["h1"][ok, None]) | (h2 != r["call"]["h2"][ok, None])
        distinct = max(len(set(zip(a.tolist(), b.tolist()))) for a, b in zip(h1, h2))
        print(f"vote {vote}: {100 * differ.mean():.1f} % of the draws differ from the call, up to {distinct} distinct pairs")
        assert differ.mean() >= 0.30 and distinct >= 8, vote


# every per-wavefront bound of k_finish_draw (16 draws per wavefront; 1, 2 and 4 wavefronts) and one past each; 48 / 49:
# the fourth wavefront without and with a draw
@pytest.mark.parametrize("n", [1, 16, 17, 32, 33, 48, 49, DRAW_MAX])
def test_spread_posteriors_at_every_draw_bound(n, spread_case):
    model, G, refs = spread_case
    for vote, (got, _) in run_case(model, G, n, what="spread", refs=refs).items():
        assert np.all(got["h1"][77] == NA) and np.all(got["prob"][77] == 0.0) and np.isnan(got["matching"][77]), vote


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
        for vote in (1, 2):
            got = dev.predict_draw(G, 7, SEED, vote)
            assert_draws_equal(got, draws(model, G, 7, SEED, vote=vote), f"drb1 vote={vote}")
            check_draws(got, dev.predict_raw(G, vote, want_dosage=False), what=f"drb1 vote={vote}")
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


def test_two_alleles_fewer_cells_than_one_unrolled_step():
    model, G = two_allele_case()
    for vote, (got, want) in run_case(model, G, 24, what="2 alleles").items():
        assert model.n_cell == 3
        assert (got["h1"][:, 0] != NA).any() and (got["h1"][:, 0] == NA).any(), vote


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


def test_nan_posteriors_give_na_draws_with_nan_probabilities():
    model, G = underflow_case()
    res = run_case(model, G, 3, what="underflow")
    got, want = res[1]
    assert np.isnan(want["postprob"][0]).all() and want["call"]["h1"][0] == NA           # the corner is there
    assert np.all(got["h1"][0] == NA) and np.all(got["h2"][0] == NA) and np.isnan(got["prob"][0]).all()
    assert np.all(got["h1"][2] == NA) and np.all(got["h2"][2] == NA) and np.all(got["prob"][2] == 0.0)     # all missing


# 6 ---------------------------------------------------------------------------------------------------------------
def test_cohort_larger_than_a_batch_host_entry_and_device_entry():
    """More samples than batch_limit(): the host entry goes through the three-stream slices, the device entry through
    several batches of one resident matrix; both equal the reference computed in one piece -- the index is global."""
    import torch
    model, founders, af = synth.make_model("hla-a-small")
    dev = hb.hlaModelFromObj(model)
    try:
        ns = dev.batch_limit() + 3017
        G, _ = synth.make_samples(founders, af, ns, seed=31)
        G[ns - 1, :] = NA
        n = 4
        want = draws(model, G, n, SEED)
        got = dev.predict_draw(G, n, SEED, 1)
        assert dev.status() == 0 and dev.handover_faults() == 0
        assert_draws_equal(got, want, "host entry")
        tdev = torch.device("cuda", dev.device())
        dg = torch.from_numpy(G).to(tdev)
        o = dict(h1=torch.empty((ns, n), dtype=torch.int32, device=tdev), h2=torch.empty((ns, n), dtype=torch.int32, device=tdev),
                 prob=torch.empty((ns, n), dtype=torch.float64, device=tdev), matching=torch.empty(ns, dtype=torch.float64, device=tdev))
        torch.cuda.synchronize(tdev)
        st = torch.cuda.current_stream(tdev)
        dev.predict_draw_device(dg.data_ptr(), ns, n, SEED, o["h1"].data_ptr(), o["h2"].data_ptr(), o["prob"].data_ptr(),
                                o["matching"].data_ptr(), vote_method=1, stream=st.cuda_stream)
        st.synchronize()
        assert dev.status() == 0
        assert_draws_equal({key: o[key].cpu().numpy() for key in o}, want, "device entry")
    finally:
        dev.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_sample0_windows_the_cohort_entry_and_the_prefix_property(spread_case):
    model, G, _ = spread_case
    a, b, n = 37, 101, 6
    dev = hb.hlaModelFromObj(model)
    try:
        whole = dev.predict_draw(G, n, SEED, 1)
        part = dev.predict_draw(G[a:b], n, SEED, 1, sample0=a)
        plain = dev.predict_draw(G[a:b], n, SEED, 1)
        for key in ("h1", "h2", "prob", "matching"):
            assert np.array_equal(part[key], whole[key][a:b], equal_nan=True), key
        assert not np.array_equal(plain["h1"], whole["h1"][a:b])                     # the argument acts
        assert np.array_equal(plain["matching"], whole["matching"][a:b], equal_nan=True)
        # a far window: an index beyond 2^32 is another stream again, and equals the reference's
        far = dev.predict_draw(G[a:b], n, SEED, 1, sample0=(1 << 32) + a)
        assert not np.array_equal(far["h1"], part["h1"])
        raw = dev.predict_raw(G[a:b], 1, want_dosage=False, want_prob=True)
        assert_draws_equal(far, draws_from_postprob(raw["postprob"], n, SEED, (1 << 32) + a, model.n_hla), "far window", keys=("h1", "h2", "prob"))
        col = np.arange(model.n_snp, dtype=np.int32)
        with hb.HlaDeviceCohort(synth.as_snp_geno(model, G)) as coh:
            win = dev.predict_draw_cohort(coh, col, None, n, SEED, 1, first=a, count=b - a, sample0=a)
            win0 = dev.predict_draw_cohort(coh, col, None, n, SEED, 1, first=a, count=b - a)
            all_ = dev.predict_draw_cohort(coh, col, None, n, SEED, 1)
        for key in ("h1", "h2", "prob", "matching"):
            assert np.array_equal(win[key], whole[key][a:b], equal_nan=True), key
            assert np.array_equal(all_[key], whole[key], equal_nan=True), key
            assert np.array_equal(win0[key], plain[key], equal_nan=True), key          # (`first` is not added)
        # the first draws of a longer list are the shorter list; another seed is another list
        for m_ in (17, DRAW_MAX):
            longer = dev.predict_draw(G, m_, SEED, 1)
            for key in ("h1", "h2", "prob"):
                assert np.array_equal(longer[key][:, :n], whole[key], equal_nan=True), (m_, key)
        assert not np.array_equal(dev.predict_draw(G, n, SEED + 1, 1)["h1"], whole["h1"])
        assert dev.status() == 0
    finally:
        dev.close()


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def benchmark_batch():
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 10_000)
    return model, G, draws(model, G, 4, SEED)


@pytest.mark.parametrize("which_pass", [1, 2])
def test_host_entry_repairs_a_dropped_handover(which_pass, benchmark_batch):
    """The benchmark batch (both passes have cut tails): with the first hand-over of a pass dropped the poisoned draws are
    never returned -- the library runs the call again without hand-overs, and the draws are what they would have been.

    "No NaN" is asked of every sample whose posterior holds none: in this batch the oracle's own posterior holds a NaN
    for two samples of the 10,000 (3110: all cells but one, 6365: every cell -- an underflow, src/LibHLA.cpp:1826-1828), and by the
    contract those are NA draws with NaN probabilities on any route; a poisoned batch would be NaN in every sample."""
    model, G, want = benchmark_batch
    m = hb.hlaModelFromObj(model)
    try:
        m.inject_handover_fault(which_pass)
        got = m.predict_draw(G, 4, SEED, 1)
        assert m.handover_faults() == 1 and m.status() == 0
    finally:
        m.close()
    nan_in_posterior = np.isnan(want["postprob"]).any(axis=1)
    assert nan_in_posterior.sum() == 2                # (a change of the synthetic batch is to be noticed)
    assert not np.isnan(got["prob"][~nan_in_posterior]).any()
    assert np.isnan(got["prob"][nan_in_posterior]).all() and np.all(got["h1"][nan_in_posterior] == NA)
    assert_draws_equal(got, want, f"repair, pass {which_pass}")


# 9 ---------------------------------------------------------------------------------------------------------------
def _assert_draws_are(d, res, n, seed, n_hla, what):
    """The reference applied to hlaPredict(type="response+prob")'s matrix [n_cell, n_samp]."""
    want = draws_from_postprob(np.ascontiguousarray(res.postprob.T), n, seed, 0, n_hla)
    want["matching"] = res.matching
    assert_draws_equal({"h1": d.h1, "h2": d.h2, "prob": d.prob, "matching": d.matching}, want, what)
    assert d.sample_id == list(res.sample_id) and d.assembly == res.assembly and d.n == n and d.seed == seed
    assert d.locus == res.locus


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
def test_hla_predict_draws_end_to_end(vote, model_a, hapmap_geno):
    n, seed = 5, 31337
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 333, seed=12, miss=0.3)
    G[5, :] = NA
    m = hb.hlaModelFromObj(model)
    try:
        # the mapped route: both memory orders of the cohort's own matrix, and the same cohort resident on the device
        snp = mapped_cohort(model, G)
        for order in ("C", "F"):
            snp.genotype = np.asarray(snp.genotype, order=order)
            with pytest.warns(UserWarning, match="No prediction output"):
                d = hb.hlaPredictDraws(m, snp, n=n, seed=seed, vote=vote, verbose=False)
            with pytest.warns(UserWarning):
                res = hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False)
            _assert_draws_are(d, res, n, seed, model.n_hla, f"HlaSNPGeno {order}")
            one = d.draw(1)
            assert d.allele1[1] == one.allele1 and d.allele2[1] == one.allele2 and d.levels == model.hla_allele
            assert [x.allele1 for x in d] == d.allele1
        with hb.HlaDeviceCohort(snp) as coh:
            with pytest.warns(UserWarning, match="No prediction output"):
                dc = hb.hlaPredictDraws(m, coh, n=n, seed=seed, vote=vote, verbose=False)
        _assert_draws_are(dc, res, n, seed, model.n_hla, "HlaDeviceCohort")
        # a numeric matrix [n.snp, n.samp] in C order and in Fortran order, and a vector
        for mat, what in ((np.ascontiguousarray(G[:100].T), "C"), (np.asfortranarray(G[:100].T), "F"),
                          (np.ascontiguousarray(G[:100].T).astype(np.float64), "float"), (G[3].copy(), "vector")):
            if what == "vector":
                d = hb.hlaPredictDraws(m, mat, n=n, seed=seed, vote=vote, verbose=False)
            else:
                with pytest.warns(UserWarning, match="No prediction output"):
                    d = hb.hlaPredictDraws(m, mat, n=n, seed=seed, vote=vote, verbose=False)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = hb.hlaPredict(m, mat, type="response+prob", vote=vote, verbose=False)
            _assert_draws_are(d, res, n, seed, model.n_hla, what)
        # seed=None: one integer from the module's stream -- reproducible behind set_seed, different from call to call
        mat = np.ascontiguousarray(G[10:100].T)
        hb.set_seed(77)
        d1 = hb.hlaPredictDraws(m, mat, n=n, vote=vote, verbose=False)
        d2 = hb.hlaPredictDraws(m, mat, n=n, vote=vote, verbose=False)
        hb.set_seed(77)
        d3 = hb.hlaPredictDraws(m, mat, n=n, vote=vote, verbose=False)
        assert d1.seed == d3.seed and d1.seed != d2.seed
        assert np.array_equal(d1.h1, d3.h1) and np.array_equal(d1.h2, d3.h2) and np.array_equal(d1.prob, d3.prob)
        assert not (np.array_equal(d1.h1, d2.h1) and np.array_equal(d1.h2, d2.h2))
        again = hb.hlaPredictDraws(m, mat, n=n, seed=d1.seed, vote=vote, verbose=False)
        assert np.array_equal(again.h1, d1.h1) and np.array_equal(again.h2, d1.h2)
    finally:
        m.close()
    # the lazily opened BED file of the HapMap fixture
    lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
    m = hb.hlaModelFromObj(model_a)
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d = hb.hlaPredictDraws(m, lazy, n=DRAW_MAX, seed=seed, vote=vote, match_type="RefSNP", verbose=False)
            res = hb.hlaPredict(m, lazy, type="response+prob", vote=vote, match_type="RefSNP", verbose=False)
        _assert_draws_are(d, res, DRAW_MAX, seed, model_a.n_hla, "BED")
    finally:
        m.close()


def test_verbose_text(model_a, hapmap_geno, capsys):
    m = hb.hlaModelFromObj(model_a)
    try:
        hb.hlaPredictDraws(m, hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(5))), n=7, seed=3, match_type="RefSNP")
    finally:
        m.close()
    text = capsys.readouterr().out
    assert "7 posterior draws per sample" in text and "seed 3" in text and "# of samples: 5" in text


# 10 --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_call(model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    ns, n = len(G), 3
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: L.hibag_hip_last_error().decode()
    h1, h2 = np.empty((ns, DRAW_MAX + 1), np.int32), np.empty((ns, DRAW_MAX + 1), np.int32)
    pr, mt = np.empty((ns, DRAW_MAX + 1)), np.empty(ns)
    col = np.arange(model_a.n_snp, dtype=np.int32)
    dev = hb.hlaModelFromObj(model_a)
    try:
        call = lambda nn, a, b, c, d, n_samp=ns, vote=1, sample0=0: L.hibag_hip_predict_draw(
            dev.handle, p(G), n_samp, vote, nn, SEED, sample0, p(a), p(b), p(c), p(d))
        entries = {
            "host": lambda nn: call(nn, h1, h2, pr, mt),
            "device": lambda nn: L.hibag_hip_predict_draw_device(dev.handle, p(G), ns, 1, nn, SEED, 0, p(h1), p(h2), p(pr), p(mt), None),
            "mapped": lambda nn: L.hibag_hip_predict_draw_mapped(dev.handle, p(G), ns, G.shape[1], p(col), None, 1, nn, SEED, 0,
                                                                 p(h1), p(h2), p(pr), p(mt)),
            "snp_major": lambda nn: L.hibag_hip_predict_draw_snp_major(dev.handle, p(G), ns, ns, G.shape[1], None, None, 1, nn, SEED, 0,
                                                                       p(h1), p(h2), p(pr), p(mt)),
            "bed": lambda nn: L.hibag_hip_predict_draw_bed(dev.handle, BED.encode(), 90, 5316, p(col), None, 1, nn, SEED, 0,
                                                           p(h1), p(h2), p(pr), p(mt)),
        }
        snp = synth.as_snp_geno(model_a, G)
        with hb.HlaDeviceCohort(snp) as coh:
            entries["cohort"] = lambda nn: L.hibag_hip_predict_draw_cohort(dev.handle, coh.handle, 0, ns, p(col), None, 1, nn, SEED, 0,
                                                                           p(h1), p(h2), p(pr), p(mt))
            for name, f in entries.items():
                for bad_n in (0, DRAW_MAX + 1):
                    assert f(bad_n) == -1 and "HIBAG_HIP_DRAW_MAX" in err() and str(DRAW_MAX) in err(), (name, bad_n)
            assert L.hibag_hip_predict_draw_cohort(dev.handle, coh.handle, 0, ns, p(col), None, 1, n, SEED, -1,
                                                   p(h1), p(h2), p(pr), p(mt)) == -1 and "sample0" in err()
        for args in ((None, h2, pr, mt), (h1, None, pr, mt), (h1, h2, None, mt)):
            assert call(n, *args) == -1 and "required" in err()
        assert call(n, h1, h2, pr, mt, n_samp=-1) == -1
        assert call(n, h1, h2, pr, mt, vote=3) == -1 and "vote_method" in err()
        assert call(n, h1, h2, pr, mt, sample0=-1) == -1 and "sample0" in err()
        assert dev.status() == 0
        # the model is still usable, and matching may be NULL
        a = np.empty((ns, n), np.int32); b = np.empty((ns, n), np.int32); c = np.empty((ns, n))
        assert call(n, a, b, c, None) == 0
        got = dev.predict_draw(G, n, SEED, 1)
        assert np.array_equal(a, got["h1"]) and np.array_equal(b, got["h2"]) and np.array_equal(c, got["prob"], equal_nan=True)
        assert_draws_equal(got, draws(model_a, G, n, SEED), "after the rejected calls")
        assert call(n, None, None, None, None, n_samp=0) == 0                          # nothing to write
    finally:
        dev.close()
