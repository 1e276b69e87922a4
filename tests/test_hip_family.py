"""hlaPredictFamily on the GPU: hibag_hip_predict_family and its routes equal, every sample and both vote methods, to the
reference (tests/family_reference.py: the contract of DESIGN.md section 19 applied to the CPU oracle's posterior matrix);
founders are predict_raw's own call, probability and dosage; independent of batches, slices, routes, rounds, a repaired
hand-over and of whether dosages were asked for; the model's other outputs untouched; invalid arguments rejected.  Every
comparison is exact equality (NaN == NaN)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import hibag_amd as hb
from conftest import REFDATA, align_geno
from family_reference import (assert_family_equal, conditional, depths, family, family_from_postprob, founders_only,
                              model_prior)
from hibag_amd import NA_INTEGER, _lib, synth
from hibag_amd.family import depth_order

pytestmark = pytest.mark.gpu

NA = NA_INTEGER
BED = os.path.join(REFDATA, "HapMap_CEU.bed")
BIM = os.path.join(REFDATA, "HapMap_CEU.bim")
FAM = os.path.join(REFDATA, "HapMap_CEU.fam")
OUT = ("h1", "h2", "prob", "support", "matching")


@pytest.fixture(scope="module", autouse=True)
def _target():
    hb.hlaSetKernelTarget("hip")


def from_oracle(ref, n_hla, rows, ped, prior):
    """The reference of the samples `rows` of an oracle result (family_reference.family's value) under another pedigree."""
    want = family_from_postprob(ref["postprob"][rows], n_hla, ped, prior)
    want["matching"] = ref["matching"][rows]
    return want


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


def run_case(model, G, ped, prior, votes=(1, 2), what="", refs=None):
    """predict_family, with and without dosages, against the reference; returns {vote: (got, want, raw)}."""
    out = {}
    dev = hb.hlaModelFromObj(model)
    try:
        for vote in votes:
            got = dev.predict_family(G, ped, prior, vote, want_dosage=True)
            lean = dev.predict_family(G, ped, prior, vote, want_dosage=False)
            raw = dev.predict_raw(G, vote, want_dosage=True)
            assert dev.status() == 0 and dev.handover_faults() == 0
            want = refs[vote] if refs is not None else family(model, G, ped, prior, vote=vote)
            check_shape(got, len(G), model.n_hla, True)
            check_shape(lean, len(G), model.n_hla, False)
            assert_family_equal(got, want, f"{what} vote={vote}")
            for key in OUT:                                   # the optional output changes nothing
                assert np.array_equal(got[key], lean[key], equal_nan=True), (what, vote, key)
            assert np.array_equal(got["matching"], raw["matching"], equal_nan=True), (what, vote)
            founders = np.all(np.asarray(ped) < 0, axis=1)    # rule 9 on every founder of every case
            for key in ("h1", "h2", "prob", "dosage"):
                assert np.array_equal(got[key][founders], raw[key][founders], equal_nan=True), (what, vote, key)
            out[vote] = (got, want, raw)
    finally:
        dev.close()
    return out


def trios_plus_one(founders, af, n_fam, seed, miss=0.85):
    """n_fam trios, parents first (synth.make_family), and one unrelated founder behind them."""
    G, truth, ped = synth.make_family(founders, af, n_fam, seed=seed, miss=miss)
    g1, t1 = synth.make_samples(founders, af, 1, seed=seed + 1, miss=miss, heavy_missing_frac=0.0)
    return (np.ascontiguousarray(np.concatenate([G, g1])), np.concatenate([truth, t1]),
            np.concatenate([ped, founders_only(1)]))


# 1 ---------------------------------------------------------------------------------------------------------------
# A row of the walk is taken in groups of eight cells: n_hla = 2 (three cells), 8 (the first row exactly one group), 9 (one
# cell more), 33 (four groups and one cell; rows of every length modulo 8).
@pytest.mark.parametrize("n", [2, 8, 9, 33])
def test_row_and_group_of_eight_tails(n):
    model, founders, af = synth.make_model("hla-a-small", seed=11, n_hla=n, n_haplo=max(40, 2 * n), n_classifier=6)
    G, _, ped = trios_plus_one(founders, af, 43, seed=12)
    assert len(G) == 130
    G[50, :] = NA                                             # the mother of child 93
    res = run_case(model, G, ped, model_prior(model), what=f"n_hla={n}")
    for vote, (got, want, raw) in res.items():
        assert got["h1"][50] == NA and got["prob"][50] == 0.0 and got["support"][50] == 0.0 and np.isnan(got["matching"][50]), vote
    got, _, raw = res[1]
    kids = np.arange(86, 129)
    differ = int(np.count_nonzero((got["h1"][kids] != raw["h1"][kids]) | (got["h2"][kids] != raw["h2"][kids])))
    print(f"n_hla={n}: {differ} of 43 children's calls differ from predict_raw's, {int((got['h1'] == NA).sum())} NA")
    assert differ >= 1


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread_case():
    """The spread model (14 alleles, 105 cells), 43 trios and a founder with 85 % of the genotypes missing; the oracle is
    run once per vote, every test below re-weights rows of its matrix."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, truth, ped = trios_plus_one(founders, af, 43, seed=12)
    q = model_prior(model)
    refs = {vote: family(model, G, ped, q, vote=vote) for vote in (1, 2)}
    return model, G, ped, q, refs


def placed(n_samp):
    """Rows of the spread case for a call of n_samp samples and its pedigree: whole trios of the case (father f, mother
    43 + f, child 86 + f) placed at chosen lanes, unrelated samples everywhere else."""
    spots = []                                                # (father's, mother's, child's position)
    if n_samp >= 3:
        spots.append((0, 1, 2))                               # a child whose parents are the call's samples 0 and 1
    if n_samp >= 63:
        spots.append((10, 5, 40))                             # all three in one wavefront, the mother first
    if n_samp >= 65:
        spots.append((62, 63, 64))                            # parents in the last lanes of a wavefront, the child in lane 0 of the next
    if n_samp >= 130:
        spots.append((70, 127, 129))                          # across the second and third wavefront
    rows = np.full(n_samp, -1, np.int64)
    ped = founders_only(n_samp)
    for f, (a, b, c) in enumerate(spots):
        rows[[a, b, c]] = (f, 43 + f, 86 + f)
        ped[c] = (a, b)
    spare = [r for r in range(130) if r % 43 >= len(spots) or r == 129]
    free = np.nonzero(rows < 0)[0]
    rows[free] = np.array(spare)[np.arange(len(free)) % len(spare)]
    return rows, ped


# lane = sample, a wavefront is 64 of them: one sample, one trio, a wavefront just not / exactly / not any more full, three
@pytest.mark.parametrize("n_samp", [1, 3, 63, 64, 65, 130])
def test_lane_mapping(n_samp, spread_case):
    model, G, _, q, refs = spread_case
    rows, ped = placed(n_samp)
    want = {vote: from_oracle(refs[vote], model.n_hla, rows, ped, q) for vote in (1, 2)}
    res = run_case(model, np.ascontiguousarray(G[rows]), ped, q, what=f"n_samp={n_samp}", refs=want)
    if n_samp >= 3:                                           # the weight is there: the child's support is not its own row's sum
        got, _, _ = res[1]
        assert got["support"][2] != np.cumsum(refs[1]["postprob"][rows[2]])[-1]


# 3 ---------------------------------------------------------------------------------------------------------------
def test_rounds_in_one_batch(spread_case):
    """Twelve samples, a four-generation chain interleaved with unrelated founders: parents precede their children but the
    depths are not sorted, so the batch takes four rounds.  The same pedigree depth-sorted gives every sample the same
    result."""
    model, G, _, q, refs = spread_case
    ped = founders_only(12)
    ped[2] = (0, 1)
    ped[4] = (2, 3)
    ped[7] = (5, 4)
    ped[8] = (6, -1)
    ped[10] = (8, 9)
    assert depths(ped).tolist() == [0, 0, 1, 0, 2, 0, 0, 3, 1, 0, 2, 0]
    rows = np.array([0, 43, 86, 44, 87, 1, 2, 88, 89, 45, 90, 129])
    want = {vote: from_oracle(refs[vote], model.n_hla, rows, ped, q) for vote in (1, 2)}
    res = run_case(model, np.ascontiguousarray(G[rows]), ped, q, what="chain", refs=want)
    # the grandchildren's weights come from WEIGHTED parents: the chain's result differs from the one with sample 4 a founder
    cut = ped.copy()
    cut[4] = (-1, -1)
    assert from_oracle(refs[1], model.n_hla, rows, cut, q)["support"][7] != want[1]["support"][7]
    # depth-sorted: one round per depth over the whole batch
    fake = ped[::-1].copy()                                   # children first: depth_order has to sort
    fake = np.where(fake >= 0, 11 - fake, -1).astype(np.int32)
    order, inverse, sorted_ped, depth = depth_order(fake)
    assert np.all(np.diff(depth[order]) >= 0) and not np.array_equal(order, np.arange(12))
    Gs = np.ascontiguousarray(G[rows][::-1][order])
    dev = hb.hlaModelFromObj(model)
    try:
        for vote in (1, 2):
            got = dev.predict_family(Gs, sorted_ped, q, vote, want_dosage=True)
            back = {k: v[inverse][::-1] for k, v in got.items()}
            for key in OUT + ("dosage",):
                assert np.array_equal(back[key], res[vote][0][key], equal_nan=True), (vote, key)
    finally:
        dev.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def assert_rule_9(model, G, what):
    """A founders-only pedigree on the device against predict_raw itself, and predict_raw identical before and after."""
    ns = len(G)
    ped = founders_only(ns)
    q = model_prior(model)
    dev = hb.hlaModelFromObj(model)
    try:
        before = {vote: dev.predict_raw(G, vote, want_dosage=True, want_prob=True) for vote in (1, 2)}
        for vote in (1, 2):
            for prior in (q, None):
                got = dev.predict_family(G, ped, prior, vote, want_dosage=True)
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


def test_founders_are_predict_raw_on_the_hla_b_shape():
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 300)
    G[0, :] = NA
    assert model.n_cell == 1275
    _, _, before = assert_rule_9(model, G, "hla-b")
    assert before[1]["h1"][0] == NA and (before[1]["h1"][1:] != NA).sum() >= 290


def test_founders_are_predict_raw_on_the_drb1_shape():
    """The large-n_cell, store-every-cell layout (pass 2 = k_accum_cells): 1,830 cells."""
    model, founders, af = synth.make_model("hla-drb1", n_classifier=8)
    G, _ = synth.make_samples(founders, af, 200)
    G[7, :] = NA
    stored, second, _ = assert_rule_9(model, G, "drb1")
    assert stored > 0 and second == 0
    # and trios on this layout
    Gt, _, ped = trios_plus_one(founders, af, 33, seed=5, miss=0.6)
    got, _, raw = run_case(model, Gt, ped, model_prior(model), votes=(1,), what="drb1 trios")[1]
    assert not np.array_equal(got["prob"][66:99], raw["prob"][66:99])


# 5 ---------------------------------------------------------------------------------------------------------------
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


def test_a_parent_without_a_prediction_is_unknown(spread_case):
    model, G, ped, q, _ = spread_case
    G = G.copy()
    G[0, :] = NA                                              # the father of child 86
    G[1, :] = NA                                              # both parents of child 87
    G[44, :] = NA
    for vote, (got, _, raw) in run_case(model, G, ped, q, what="all-NA parents").items():
        assert got["support"][0] == 0.0 and got["support"][1] == 0.0 and got["support"][44] == 0.0
        for key in ("h1", "h2", "prob", "dosage"):            # both parents unknown: the child's own call
            assert np.array_equal(got[key][87], raw[key][87], equal_nan=True), (vote, key)
        duo = ped.copy()
        duo[86, 0] = -1
        duo[87] = (-1, -1)
        dev = hb.hlaModelFromObj(model)
        try:
            again = dev.predict_family(G, duo, q, vote, want_dosage=True)
        finally:
            dev.close()
        for key in OUT + ("dosage",):                         # one parent unknown: the duo's result
            assert np.array_equal(got[key], again[key], equal_nan=True), (vote, key)
        assert got["prob"][86] != raw["prob"][86]             # ... in which the mother still counts


def test_nan_rows_are_unknown_parents_and_never_called_children():
    model, G3 = underflow_case()
    good = np.full((1, G3.shape[1]), NA, np.int32)            # only the near classifier's SNPs typed: a posterior
    good[0, :4] = (0, 1, 0, 1)
    #            0: NaN row   1: a posterior   2: all missing   3: child of (0, 1)   4: NaN child of (1, 3)   5: child of (0, 2)
    G = np.ascontiguousarray(np.concatenate([G3, good])[[0, 3, 2, 3, 0, 3]])
    ped = np.array([[-1, -1], [-1, -1], [-1, -1], [0, 1], [1, 3], [0, 2]], np.int32)
    q = model_prior(model)
    got, want, raw = run_case(model, G, ped, q, votes=(1,), what="underflow")[1]
    assert np.isnan(want["postprob"][0]).all() and want["call"]["h1"][0] == NA                 # the corner is there
    assert np.isnan(got["support"][0]) and got["h1"][0] == NA and got["prob"][0] == 0.0
    duo = family_from_postprob(want["postprob"], 3, np.array([[-1, -1]] * 3 + [[-1, 1], [1, 3], [-1, -1]]), q)
    for key in ("h1", "h2", "prob", "support", "dosage"):     # the NaN father is unknown; NaN and all-missing parents: the own call
        assert np.array_equal(got[key][3], duo[key][3], equal_nan=True) and np.array_equal(got[key][5], duo[key][5], equal_nan=True), key
    assert got["h1"][3] != NA and got["support"][3] > 0 and got["prob"][3] != raw["prob"][3]     # (the mother counts)
    assert got["h1"][4] == NA and got["prob"][4] == 0.0 and np.isnan(got["support"][4]) and np.isnan(got["dosage"][4]).all()
    for key in ("h1", "h2", "prob", "dosage"):
        assert np.array_equal(got[key][5], raw[key][5], equal_nan=True), key


def test_two_alleles_three_cells_every_trio_of_rows():
    model, G6 = two_allele_case()
    assert model.n_cell == 3
    trios = [(f, m, c) for f in range(6) for m in range(6) for c in range(6)]
    G = np.ascontiguousarray(np.concatenate([G6, G6[[c for _, _, c in trios]]]))
    ped = np.concatenate([founders_only(6), np.array([(f, m) for f, m, _ in trios], np.int32)])
    assert len(G) == 222
    for prior in (model_prior(model), None):
        for vote, (got, _, raw) in run_case(model, G, ped, prior, what="2 alleles").items():
            assert (got["h1"] != NA).any() and (got["h1"] == NA).any(), vote
            assert not np.array_equal(got["prob"][6:], raw["prob"][6:])


# 6 ---------------------------------------------------------------------------------------------------------------
def laid_out(n_fam, n_samp, seed, fixed=(), head=0):
    """Where the rows of `n_fam` parents-first trios (father f, mother n_fam + f, child 2 n_fam + f) and of the
    n_samp - 3 n_fam unrelated rows behind them stand in a call of n_samp samples, and the call's pedigree:
    families 0 .. head - 1 keep their parents at the start of the call and get their children at its end; `fixed`: (family,
    (father's, mother's, child's position)); everybody else is shuffled under the one rule that parents precede children."""
    rng = np.random.default_rng(seed)
    row_at = np.full(n_samp, -1, np.int64)                    # which base row stands at a position
    trio_at = {}
    for f in range(head):
        trio_at[f] = (f, head + f, n_samp - head + f)
    for f, spots in fixed:
        trio_at[f] = spots
    taken = {p for spots in trio_at.values() for p in spots}
    assert len(taken) == 3 * len(trio_at)
    free = [int(p) for p in rng.permutation(n_samp) if int(p) not in taken]
    for f in range(n_fam):
        if f not in trio_at:
            a, b, c = sorted(free[-3:])
            del free[-3:]
            trio_at[f] = (a, b, c) if rng.random() < 0.5 else (b, a, c)
    ped = founders_only(n_samp)
    for f, (a, b, c) in trio_at.items():
        row_at[[a, b, c]] = (f, n_fam + f, 2 * n_fam + f)
        ped[c] = (a, b)
    row_at[np.array(free, np.int64)] = np.arange(3 * n_fam, n_samp)
    assert np.array_equal(np.sort(row_at), np.arange(n_samp))
    return row_at, ped


def family_cohort(model, founders, af, n_samp, seed, miss=0.6):
    nf = n_samp // 3
    G, _, _ = synth.make_family(founders, af, nf, seed=seed, miss=miss)
    rest, _ = synth.make_samples(founders, af, n_samp - 3 * nf + 1, seed=seed + 1, miss=miss)
    return nf, np.concatenate([G, rest[:n_samp - 3 * nf]])


def test_cohort_larger_than_a_batch_host_entry_and_device_entry():
    """More samples than batch_limit(): the host entry goes through the three-stream slices, the device entry through
    several batches of one resident matrix; parents at the start of the call with their children at its end, one trio
    across the batch boundary, everybody else shuffled.  Both equal the reference computed in one piece."""
    import torch
    model, founders, af = synth.make_model("hla-a-small")
    n = model.n_hla
    q = model_prior(model)
    dev = hb.hlaModelFromObj(model)
    try:
        lim = dev.batch_limit()
        ns = lim + 3017
        nf, base = family_cohort(model, founders, af, ns, seed=31)
        row_at, ped = laid_out(nf, ns, seed=32, fixed=[(200, (lim - 2, lim - 1, lim))], head=100)
        assert ped[lim].tolist() == [lim - 2, lim - 1] and ped[ns - 1].tolist() == [99, 199]
        G = np.ascontiguousarray(base[row_at])
        G[ns - 2, :] = NA
        want = family(model, G, ped, q)
        got = dev.predict_family(G, ped, q, 1, want_dosage=True)
        assert dev.status() == 0 and dev.handover_faults() == 0
        assert_family_equal(got, want, "host entry")
        tdev = torch.device("cuda", dev.device())
        dg = torch.from_numpy(G).to(tdev)
        f64 = dict(dtype=torch.float64, device=tdev)
        o = dict(h1=torch.empty(ns, dtype=torch.int32, device=tdev), h2=torch.empty(ns, dtype=torch.int32, device=tdev),
                 prob=torch.empty(ns, **f64), support=torch.empty(ns, **f64), matching=torch.empty(ns, **f64),
                 dosage=torch.empty((ns, n), **f64))
        torch.cuda.synchronize(tdev)
        st = torch.cuda.current_stream(tdev)
        dev.predict_family_device(dg.data_ptr(), ns, ped, q, o["h1"].data_ptr(), o["h2"].data_ptr(), o["prob"].data_ptr(),
                                  o["support"].data_ptr(), o["matching"].data_ptr(), o["dosage"].data_ptr(), vote_method=1,
                                  stream=st.cuda_stream)
        st.synchronize()
        assert dev.status() == 0
        assert_family_equal({key: o[key].cpu().numpy() for key in o}, want, "device entry")
    finally:
        dev.close()


def test_slices_of_64(spread_case, monkeypatch):
    """200 samples cut into slices of 64 (the three-stream pipeline): parents and children in different slices."""
    model, _, _, q, _ = spread_case
    _, founders, af = synth.make_model("hla-a-small", seed=11)
    nf, base = family_cohort(model, founders, af, 200, seed=41, miss=0.85)
    row_at, ped = laid_out(nf, 200, seed=42, head=10)
    G = np.ascontiguousarray(base[row_at])
    want = {vote: family(model, G, ped, q, vote=vote) for vote in (1, 2)}
    assert np.count_nonzero((ped[:, 0] >= 0) & (ped[:, 0] // 64 != np.arange(200) // 64)) >= 10
    monkeypatch.setenv("HIBAG_STAGED_SLICE", "64")
    run_case(model, G, ped, q, what="slices of 64", refs=want)


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def benchmark_batch():
    model, founders, af = synth.make_model("hla-b")
    G, _, ped = trios_plus_one(founders, af, 3333, seed=synth.DEFAULT_SEED + 2, miss=0.01)
    q = model_prior(model)
    return model, G, ped, q, family(model, G, ped, q)


def test_host_entry_repairs_a_dropped_handover(benchmark_batch):
    """The benchmark batch (both passes have cut tails): with the first hand-over of pass 1 dropped the poisoned calls are
    never returned, and no child is weighted with a poisoned parent -- the library runs the call again without hand-overs,
    pedigree, prior and the parents' results with it."""
    model, G, ped, q, want = benchmark_batch
    assert len(G) == 10_000
    m = hb.hlaModelFromObj(model)
    try:
        m.inject_handover_fault(1)
        got = m.predict_family(G, ped, q, 1, want_dosage=True)
        assert m.handover_faults() == 1 and m.status() == 0
    finally:
        m.close()
    assert_family_equal(got, want, "repair, pass 1")


# 8 ---------------------------------------------------------------------------------------------------------------
def mapped_cohort(model, G, sample_id):
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
    return hb.HlaSNPGeno(genotype=np.array([rows[i] for i in order], np.int32), sample_id=list(sample_id),
                         snp_id=[ids[i] for i in order], snp_position=np.array([pos[i] for i in order], np.float64),
                         snp_allele=[alle[i] for i in order], assembly="hg19")


def _assert_family_is(r, res, base_ped, perm, prior, what, want_dosage):
    """The reference applied to hlaPredict(type="response+prob")'s matrix [n_cell, n_samp] in the parents-first base order
    (caller position i holds base sample perm[i]), then rule 7, back in the caller's order."""
    n_hla = len(r.alleles)
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    base = family_from_postprob(np.ascontiguousarray(res.postprob.T)[inv], n_hla, base_ped, prior)
    want = {k: v[perm] for k, v in base.items()}
    want["matching"] = res.matching
    got = {"h1": r.h1, "h2": r.h2, "prob": r.prob_joint, "support": r.support, "matching": r.matching}
    assert_family_equal(got, want, what, keys=OUT)
    cond = conditional(want)
    assert np.array_equal(r.prob, cond["prob"], equal_nan=True), what
    assert (r.dosage is not None) == want_dosage
    if want_dosage:
        assert r.dosage.shape == (n_hla, len(r.sample_id)) and np.array_equal(r.dosage, cond["dosage"].T, equal_nan=True), what
    assert r.sample_id == list(res.sample_id) and r.assembly == res.assembly and r.locus == res.locus
    assert np.array_equal(r.pedigree, np.where(base_ped[perm] >= 0, inv[np.maximum(base_ped[perm], 0)], -1)), what
    assert np.array_equal(r.depth, depths(base_ped)[perm]), what
    calls = r.calls()
    assert calls.allele1 == [None if h == NA else r.alleles[h] for h in r.h1] and calls.prob is r.prob


@pytest.mark.parametrize("vote", ["prob", "majority"])
def test_hla_predict_family_end_to_end(vote):
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    n = model.n_hla
    G0, truth, ped0 = synth.make_family(founders, af, 60, seed=12, miss=0.85)
    G0[5, :] = NA                                             # a father without a prediction
    ns = len(G0)
    perm = np.concatenate([np.random.default_rng(3).permutation(np.arange(60, ns)), np.arange(60)])     # fathers last
    ids = [f"p{b}" for b in perm]                             # caller position i holds base sample perm[i]
    pedigree = hb.HlaPedigree([f"p{b}" for b in range(120, ns)] + ["elsewhere"], [f"p{b}" for b in range(60)] + ["nobody"],
                              [f"p{b}" for b in range(60, 120)] + [None])
    caller_ped = pedigree.indices_for(ids)
    assert np.any(caller_ped[:, 0] > np.arange(ns))           # children stand before their fathers
    q = hb.hlaModelAllelePrior(model)
    assert np.array_equal(q, model_prior(model))
    m = hb.hlaModelFromObj(model)
    try:
        snp = mapped_cohort(model, G0[perm], ids)
        for order in ("C", "F"):
            snp.genotype = np.asarray(snp.genotype, order=order)
            with pytest.warns(UserWarning):
                res = hb.hlaPredict(m, snp, type="response+prob", vote=vote, verbose=False)
            for prior, pr in (("model", q), (None, None), (np.full(n, 0.25), np.full(n, 0.25))):
                with pytest.warns(UserWarning, match="No prediction output"):
                    r = hb.hlaPredictFamily(m, snp, pedigree, prior=prior, dosage=True, vote=vote, verbose=False)
                _assert_family_is(r, res, ped0, perm, pr, f"HlaSNPGeno {order} prior={prior if isinstance(prior, str) else pr is not None}", True)
        with pytest.warns(UserWarning):
            r = hb.hlaPredictFamily(m, snp, pedigree, vote=vote, verbose=False)
        _assert_family_is(r, res, ped0, perm, q, "no dosage", False)
        # the parents' rows are hlaPredict's own
        parents = np.nonzero(r.depth == 0)[0]
        assert len(parents) == 120
        assert np.array_equal(r.h1[parents], res.h1[parents]) and np.array_equal(r.h2[parents], res.h2[parents])
        assert np.array_equal(r.prob_joint[parents], res.prob[parents], equal_nan=True)
        where5 = int(np.nonzero(perm == 5)[0][0])
        assert r.h1[where5] == NA and r.calls().allele1[where5] is None
        # fewer Mendelian-inconsistent trios than hlaPredict's calls have
        before, after = hb.hlaMendelCheck(res, pedigree), hb.hlaMendelCheck(r, pedigree)
        print(f"vote={vote}: inconsistent trios {before.n_inconsistent_trios} -> {after.n_inconsistent_trios} of {before.n_checked} checked")
        assert after.n_inconsistent_trios < before.n_inconsistent_trios and before.n_checked >= 55
        # matrices and a vector carry no sample ids: the pedigree is an integer array over the samples in order
        first = np.arange(100)
        local = np.where(caller_ped[:100] < 100, caller_ped[:100], -1).astype(np.int32)
        lorder, linv, lsorted, _ = depth_order(local)
        for mat, what in ((np.ascontiguousarray(G0[perm][:100].T), "C"), (np.asfortranarray(G0[perm][:100].T), "F"),
                          (np.ascontiguousarray(G0[perm][:100].T).astype(np.float64), "float"), (G0[perm][3].copy(), "vector")):
            lp = local if what != "vector" else founders_only(1)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = hb.hlaPredictFamily(m, mat, lp, dosage=(what != "F"), vote=vote, verbose=False)
                res = hb.hlaPredict(m, mat, type="response+prob", vote=vote, verbose=False)
            if what == "vector":
                _assert_family_is(r, res, founders_only(1), np.arange(1), q, what, True)
            else:
                _assert_family_is(r, res, lsorted, linv, q, what, what != "F")      # (caller position i holds sorted sample linv[i])
        with pytest.raises(TypeError, match="HlaSNPGeno"):
            hb.hlaPredictFamily(m, np.ascontiguousarray(G0.T), pedigree, verbose=False)
    finally:
        m.close()


def test_verbose_text_and_refused_sources(model_a, hapmap_geno, capsys, tmp_path):
    m = hb.hlaModelFromObj(model_a)
    ped = np.array([[-1, -1], [-1, -1], [0, 1], [2, -1], [-1, -1]], np.int32)
    try:
        five = hb.hlaGenoSubset(hapmap_geno, samp_sel=list(range(5)))
        hb.hlaPredictFamily(m, five, ped, match_type="RefSNP")
        text = capsys.readouterr().out
        assert "weighted by the parents' posteriors" in text and "# of samples: 5" in text
        assert "Pedigree: 1 trios, 1 duos, 3 founders; deepest generation 2" in text
        lazy = hb.hlaBED2Geno(BED, FAM, BIM, assembly="hg19", verbose=False, lazy=True)
        with pytest.raises(TypeError, match="hlaBED2Geno"):
            hb.hlaPredictFamily(m, lazy, founders_only(len(lazy.sample_id)), verbose=False)
        with hb.HlaDeviceCohort(five) as coh:
            with pytest.raises(TypeError, match="hlaBED2Geno"):
                hb.hlaPredictFamily(m, coh, ped, verbose=False)
        # the fixture's .fam file names no parents: everybody is a founder, and the calls are hlaPredict's own
        fam = hb.hlaPedigreeFromFam(FAM)
        assert len(fam) == 90 and np.all(fam.indices_for(list(hapmap_geno.sample_id)) == -1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictFamily(m, hapmap_geno, fam, match_type="RefSNP", verbose=False)
            res = hb.hlaPredict(m, hapmap_geno, match_type="RefSNP", verbose=False)
        assert r.depth.max() == 0 and np.array_equal(r.h1, res.h1) and np.array_equal(r.prob_joint, res.prob, equal_nan=True)
    finally:
        m.close()


# 9 ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_through_the_c_call(model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:10]
    ns, n = len(G), model_a.n_hla
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    err = lambda: L.hibag_hip_last_error().decode()
    ped = founders_only(ns)
    ped[4] = (1, 3)
    ped[9] = (4, -1)
    q = model_prior(model_a)
    h1, h2 = np.empty(ns, np.int32), np.empty(ns, np.int32)
    pr, sp, mt, ds = np.empty(ns), np.empty(ns), np.empty(ns), np.empty((ns, n))
    col = np.arange(model_a.n_snp, dtype=np.int32)
    dev = hb.hlaModelFromObj(model_a)
    try:
        def entries(m, pd, pq, o1, o2, o3, o4, vote=1):
            return {
                "host": lambda: L.hibag_hip_predict_family(m, p(G), ns, vote, p(pd), p(pq), p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
                "device": lambda: L.hibag_hip_predict_family_device(m, p(G), ns, vote, p(pd), p(pq), p(o1), p(o2), p(o3), p(o4),
                                                                    p(mt), p(ds), None),
                "mapped": lambda: L.hibag_hip_predict_family_mapped(m, p(G), ns, G.shape[1], p(col), None, vote, p(pd), p(pq),
                                                                    p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
                "snp_major": lambda: L.hibag_hip_predict_family_snp_major(m, p(G), ns, ns, G.shape[1], None, None, vote, p(pd), p(pq),
                                                                          p(o1), p(o2), p(o3), p(o4), p(mt), p(ds)),
            }

        # an unfinalized model
        fresh = C.c_void_p(L.hibag_hip_model_new(n, model_a.n_snp))
        assert fresh.value
        for name, f in entries(fresh, ped, q, h1, h2, pr, sp).items():
            assert f() == -1 and "not finalized" in err(), name
        L.hibag_hip_model_free(fresh)
        for name, f in entries(dev.handle, None, q, h1, h2, pr, sp).items():
            assert f() == -1 and "pedigree is NULL" in err(), name
        for s, k, v in ((4, 0, 4), (4, 1, 7), (0, 0, 0), (6, 1, -2), (9, 0, ns)):     # the sample itself, a later one, below -1
            bad = ped.copy()
            bad[s, k] = v
            for name, f in entries(dev.handle, bad, q, h1, h2, pr, sp).items():
                assert f() == -1 and f"pedigree[{s}][{k}] = {v}" in err() and "precede" in err(), (name, s, k, v)
        for v in (0.0, -0.5, float("nan"), float("inf")):
            bad = q.copy()
            bad[n - 1] = v
            for name, f in entries(dev.handle, ped, bad, h1, h2, pr, sp).items():
                assert f() == -1 and f"prior[{n - 1}]" in err() and "finite and > 0" in err(), (name, v)
        for missing in range(4):
            outs = [h1, h2, pr, sp]
            outs[missing] = None
            for name, f in entries(dev.handle, ped, q, *outs).items():
                assert f() == -1 and "required" in err(), (name, missing)
        for name, f in entries(dev.handle, ped, q, h1, h2, pr, sp, vote=3).items():
            assert f() == -1 and "vote_method" in err(), name
        assert L.hibag_hip_predict_family(None, p(G), ns, 1, p(ped), p(q), p(h1), p(h2), p(pr), p(sp), None, None) == -1
        assert L.hibag_hip_predict_family(dev.handle, p(G), -1, 1, p(ped), p(q), p(h1), p(h2), p(pr), p(sp), None, None) == -1
        assert dev.status() == 0
        # the model is still usable; prior, matching and dosage may be NULL; n_samp == 0 with NULL pointers is fine
        call = lambda pq, a, b: L.hibag_hip_predict_family(dev.handle, p(G), ns, 1, p(ped), p(pq), p(h1), p(h2), p(pr), p(sp), p(a), p(b))
        want = family(model_a, G, ped, q)
        assert call(q, None, None) == 0
        assert_family_equal({"h1": h1, "h2": h2, "prob": pr, "support": sp}, want, "after the rejected calls", keys=("h1", "h2", "prob", "support"))
        assert call(q, mt, ds) == 0
        assert_family_equal({"h1": h1, "h2": h2, "prob": pr, "support": sp, "matching": mt, "dosage": ds}, want, "after the rejected calls")
        assert call(None, mt, ds) == 0
        assert_family_equal({"h1": h1, "h2": h2, "prob": pr, "support": sp, "matching": mt, "dosage": ds},
                            family_from_postprob(want["postprob"], n, ped, None) | {"matching": want["matching"]}, "NULL prior")
        assert L.hibag_hip_predict_family(dev.handle, None, 0, 1, None, None, None, None, None, None, None, None) == 0
        assert L.hibag_hip_predict_family_device(dev.handle, None, 0, 1, None, None, None, None, None, None, None, None, None) == 0
        assert dev.status() == 0
        # the Python layer says the same in its own words
        with pytest.raises(ValueError):
            dev.predict_family(G, ped[:5], q)                              # fewer rows than samples
        with pytest.raises(ValueError):
            dev.predict_family(G, ped.astype(np.float64), q)
        with pytest.raises(ValueError):
            dev.predict_family(G, ped, q[:-1])
        with pytest.raises(hb.HibagHipError):
            dev.predict_family(G, ped[::-1].copy(), q)                     # children first: the C call's own rejection
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, ped[:5], verbose=False)
        with pytest.raises(TypeError):
            hb.hlaPredictFamily(dev, G.T, ped.astype(np.float64), verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, ped, prior=np.zeros(n), verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, ped, prior="flat", verbose=False)
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, np.array([[1, -1], [0, -1]] + [[-1, -1]] * 8), verbose=False)      # a cycle
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, np.array([[-1, -1], [0, 0]] + [[-1, -1]] * 8), verbose=False)      # father == mother
        with pytest.raises(ValueError):
            hb.hlaPredictFamily(dev, G.T, ped, vote="mean", verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = hb.hlaPredictFamily(dev, G.T, ped, prior=q, dosage=True, verbose=False)
        assert_family_equal({"h1": r.h1, "h2": r.h2, "prob": r.prob_joint, "support": r.support, "matching": r.matching}, want,
                            "after the rejected calls", keys=OUT)
    finally:
        dev.close()
