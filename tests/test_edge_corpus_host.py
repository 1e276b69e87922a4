"""The edge cases of ``ref_cases.PREDICT_CASES`` are what tests/test_hip_edge_corpus.py needs them to be (CPU, from the
references alone): the subnormal total gives a call with prob = inf, every 64-sample group of ``mixed-lanes`` holds lanes
without a call, with a finite call and with prob = inf side by side -- in the ensemble for every curve size from 4 to 12, and
per classifier for every classifier whose frequencies are scaled down --, a mask heals some poisoned lanes and leaves
others, and a merge meets posterior columns that are NaN in some rows only; for the entries with a finish of their own
(top-k, draws, groups, given, family): rows with inf cells, with inf and NaN cells, all-NaN and healthy rows share a
64-sample group, inf rows tie across top-k's segments, draws meet S = inf and S = NaN, allele sets move a call off an inf cell
or leave it NaN cells only, and a pedigree pairs every kind of parent over two generations.  These are conditions on the
inputs: where a recipe misses one, the recipe changes (seed, rate, factor), never the condition."""

import numpy as np
import pytest

import draws_reference as DR
import edge_corpus as EC
import family_reference as FR
import ref_cases as RC
import topk_reference as TR
from hibag_amd import NA_INTEGER

GROUPS = [slice(0, 64), slice(64, 128), slice(128, 192)]
RAGGED = slice(192, 200)


def _counts(h1, prob, rows):
    return tuple(int(k[rows].sum()) for k in RC.lane_kinds(h1, prob))


def test_cases_are_in_the_pinned_corpus():
    assert set(EC.NEW_CASES) <= set(RC.PREDICT_CASES) and len(RC.PREDICT_CASES) == 10


def test_subnormal_total_gives_a_call_with_infinite_probability():
    model, G = EC.case("subnormal")
    assert G.shape == (4, 32) and [len(c.snpidx) for c in model.classifiers] == [4, 32]
    r = EC.plain_want("subnormal", 1)
    assert (r["h1"][0], r["h2"][0]) == (0, 0) and np.isposinf(r["prob"][0])
    assert np.isposinf(r["postprob"][0]).all()                       # every pair of `sub` exists: inf everywhere, NaN nowhere
    for s in (1, 3):
        assert r["h1"][s] != NA_INTEGER and np.isfinite(r["prob"][s]) and np.isfinite(r["postprob"][s]).all(), s
    assert r["h1"][2] == NA_INTEGER and r["h2"][2] == NA_INTEGER and r["prob"][2] == 0 and np.isnan(r["matching"][2])
    assert np.isfinite(r["matching"][[0, 1, 3]]).all()
    # `sub` alone, everybody out of bag
    oob = EC.oob_want("subnormal", "all-out")
    assert (oob["h1"][1, 0], oob["h2"][1, 0]) == (0, 0) and np.isposinf(oob["prob"][1, 0])
    assert np.isfinite(oob["prob"][1, [1, 3]]).all() and (oob["h1"][1, [1, 3]] != NA_INTEGER).all()
    assert oob["h1"][1, 2] == NA_INTEGER and oob["prob"][1, 2] == 0
    # and in the curve: size 1 (`near` alone) is healthy, size 2 is the call above
    cur = EC.curve_want("subnormal")
    assert np.isfinite(cur["prob"][0, [0, 1, 3]]).all() and np.isposinf(cur["prob"][1, 0])


def test_subnormal_lanes_mix_the_four_samples_in_one_group():
    assert len(EC.case("subnormal-lanes")[1]) == 72
    r = EC.plain_want("subnormal-lanes", 1)
    for rows in (slice(0, 64), slice(64, 72)):
        na, fin, inf = _counts(r["h1"], r["prob"], rows)
        assert na >= 1 and fin >= 2 and inf >= 1, (rows, na, fin, inf)


def test_mixed_lanes_ensemble_every_group_holds_every_lane_kind():
    model, G = EC.case("mixed-lanes")
    assert G.shape == (200, 160) and [len(c.snpidx) for c in model.classifiers] == RC.MIXED_COUNTS
    assert (G[RC.MIXED_ALL_MISSING] == NA_INTEGER).all()
    cur = EC.curve_want("mixed-lanes")
    for size in range(4, 13):
        h1, prob = cur["h1"][size - 1], cur["prob"][size - 1]
        for g in GROUPS:
            na, fin, inf = _counts(h1, prob, g)
            assert na >= 5 and fin >= 5 and inf >= 5, (size, g, na, fin, inf)
        na, fin, _ = _counts(h1, prob, RAGGED)
        assert na >= 1 and fin >= 1, (size, na, fin)
    assert np.isnan(cur["matching"][:, RC.MIXED_ALL_MISSING]).all()


def test_mixed_lanes_per_classifier_every_group_holds_every_lane_kind():
    model, G = EC.case("mixed-lanes-each")
    oob = EC.oob_want("mixed-lanes-each", "all-out")
    for c in RC.MIXED_PER_CLASSIFIER["scaled"]:
        idx = np.asarray(model.classifiers[c].snpidx)
        typed = ((G[:, idx] >= 0) & (G[:, idx] <= 2)).any(axis=1)         # (weight > 0)
        na, fin, inf = RC.lane_kinds(oob["h1"][c], oob["prob"][c])
        for g in GROUPS:
            assert (na & typed)[g].any() and fin[g].any() and inf[g].any(), (c, g)
    # the knock-out's cut keeps a scaled classifier of each kind of width
    assert set(EC.KNOCK_CUT) <= set(RC.MIXED_PER_CLASSIFIER["scaled"])
    assert [RC.MIXED_COUNTS[c] for c in EC.KNOCK_CUT] == [12, 40, 31, 113]
    # ... and its own out-of-bag lanes (a seeded bootstrap) still hold every kind for each of them
    kmodel, _, _ = EC.knock_case("mixed-lanes-each")
    raw = EC.knock_want("mixed-lanes-each")
    nv = raw["n_variant"]
    for c, cls in enumerate(kmodel.classifiers):
        out = np.asarray(cls.samp_num) == 0
        na, fin, inf = RC.lane_kinds(raw["h1"][nv + c], raw["prob"][nv + c])
        assert (na & out).any() and (fin & out).any() and (inf & out).any(), c
    # a knock-out moves lanes between the kinds: some row's inf lanes differ from its base row's
    base_inf = np.isposinf(raw["prob"][nv + raw["classifier"]])
    assert (np.isposinf(raw["prob"][:nv]) != base_inf).any(axis=1).sum() >= 10


def test_mask_heals_some_poisoned_lanes_and_leaves_others():
    use = EC.mask("mixed-lanes")
    scaled = sorted(RC.MIXED_ENSEMBLE["scaled"])
    full = EC.plain_want("mixed-lanes", 1)
    poisoned = full["h1"] == NA_INTEGER
    poisoned[RC.MIXED_ALL_MISSING] = False                                # (no SNP: nothing to heal)
    out = ~use[scaled].any(axis=0)
    want = EC.masked_want("mixed-lanes", 1)
    na, fin, _ = RC.lane_kinds(want["h1"], want["prob"])
    healed = poisoned & out & fin & use.any(axis=0)
    stays = poisoned & ~out & na
    assert healed.sum() >= 10 and stays.sum() >= 10, (int(healed.sum()), int(stays.sum()))
    assert np.isfinite(want["postprob"][healed]).all() and np.isnan(want["postprob"][stays]).any(axis=1).all()
    # the majority vote passes over a classifier without a call: the lanes that stay poisoned above get a call from it
    vote2 = EC.masked_want("mixed-lanes", 2)
    assert (vote2["h1"][stays] != NA_INTEGER).sum() >= 10


def test_merge_meets_columns_that_are_nan_in_some_rows_only():
    partial, inf_before = 0, 0
    for name in EC.CASES:
        plan, pp, mt = EC.merge_inputs(name)
        assert 0 < len(set(plan.row_of_cell[0]) & set(plan.row_of_cell[1])) < min(len(r) for r in plan.row_of_cell), name
        for use_matching in (True, False):
            nan = np.isnan(EC.merge_want(name, use_matching)["postprob"])
            some = nan.any(axis=0) & ~nan.all(axis=0)
            if name == "subnormal-lanes":
                assert some.sum() >= 5, (name, use_matching, int(some.sum()))
            partial += int(some.sum())
        # an inf posterior entry under a finite positive weight is an inf sum before the normalisation
        inf_before += int((np.isposinf(pp[0]).any(axis=0) & np.isfinite(mt[0]) & (mt[0] > 0)).sum())
    assert partial >= 5 and inf_before >= 1, (partial, inf_before)
    # mixed-lanes brings inf next to NaN in one column (the whole merged column is NaN then), and healthy columns
    _, pp, _ = EC.merge_inputs("mixed-lanes")
    assert (np.isposinf(pp[0]).any(axis=0) & np.isnan(pp[0]).any(axis=0)).sum() >= 5
    assert np.isfinite(EC.merge_want("mixed-lanes", True)["postprob"]).all(axis=0).sum() >= 5


@pytest.mark.parametrize("name", EC.CASES)
def test_every_reference_runs_on_every_case(name):
    """Each entry's reference result has the entry's shape on every case (the GPU tests compare against exactly these)."""
    model, G = EC.case(name)
    C, n = len(model.classifiers), len(G)
    assert EC.curve_want(name)["prob"].shape == (C, n)
    for boot in ("seeded", "all-out"):
        assert EC.oob_want(name, boot)["prob"].shape == (C, n)
    kmodel, _, truth = EC.knock_case(name)
    raw = EC.knock_want(name)
    assert raw["prob"].shape == (raw["n_variant"] + len(kmodel.classifiers), n) and truth.shape == (n, 2)
    assert raw["n_variant"] == sum(len(c.snpidx) for c in kmodel.classifiers)
    for vote in (1, 2):
        assert EC.masked_want(name, vote)["postprob"].shape == (n, model.n_cell)
    assert EC.merge_want(name, True)["postprob"].shape[1] == n


# ---- top-k, draws, groups, given, family: the entries whose finish is a kernel of its own -----------------------------------
VOTES = (1, 2)


def _inf_rows(name, vote=1):
    return np.isposinf(EC.posterior(name, vote)[0]).any(axis=1)


def test_inf_nan_and_healthy_rows_share_a_group_and_the_subnormal_inf_rows_tie():
    pp, _ = EC.posterior("mixed-lanes", 1)
    kind = EC.row_kinds("mixed-lanes")
    both = np.isposinf(pp).any(axis=1) & np.isnan(pp).any(axis=1)
    assert np.array_equal(both, kind == EC.INF) and np.isnan(pp[kind == EC.NAN]).all()       # inf comes with NaN; NaN rows are all NaN
    full = [g for g in GROUPS if both[g].any() and (kind[g] == EC.NAN).any() and (kind[g] == EC.HEALTHY).any()]
    assert full, [np.bincount(kind[g], minlength=4).tolist() for g in GROUPS]
    assert both.sum() >= 5 and _inf_rows("mixed-lanes-each").any()
    for vote in VOTES[1:]:                                    # the majority vote passes over a classifier without a call
        for name in EC.CASES:
            assert np.isfinite(EC.posterior(name, vote)[0]).all(), (name, vote)
    # subnormal-lanes: inf in every cell, so every rank of the list is decided by cell order alone
    pp, _ = EC.posterior("subnormal-lanes", 1)
    rows = _inf_rows("subnormal-lanes")
    assert rows.sum() >= 10 and np.isposinf(pp[rows]).all() and rows[:64].any() and rows[64:].any()
    want = EC.topk_want("subnormal-lanes", 1, 16)
    h1, h2 = TR.pair_of_cell(np.arange(pp.shape[1]), EC.n_hla("subnormal-lanes"))
    assert (want["h1"][rows, :len(h1)] == h1).all() and (want["h2"][rows, :len(h1)] == h2).all()
    assert np.isposinf(want["prob"][rows, :len(h1)]).all() and (want["h1"][rows, len(h1):] == NA_INTEGER).all()


def test_topk_rank_0_on_inf_rows_is_the_oracles_call():
    seen = 0
    for name in EC.CASES:
        rows = _inf_rows(name)
        call = EC.plain_want(name, 1)
        for k in EC.TOPK_K:
            want = EC.topk_want(name, 1, k)
            assert np.array_equal(want["h1"][rows, 0], call["h1"][rows]) and np.array_equal(want["h2"][rows, 0], call["h2"][rows]), (name, k)
            assert np.isposinf(want["prob"][rows, 0]).all() and np.isposinf(call["prob"][rows]).all(), (name, k)
        seen += int(rows.sum())
    assert seen >= 20


def test_select_and_select_fast_agree_on_every_corpus_posterior():
    for name in EC.CASES:
        for vote in VOTES:
            pp, _ = EC.posterior(name, vote)
            for k in (1, 4, 16):
                TR.assert_topk_equal(TR.select_fast(pp, k, EC.n_hla(name)), EC.topk_want(name, vote, k) if k in EC.TOPK_K
                                     else TR.select(pp, k, EC.n_hla(name)), f"{name}, vote {vote}, k {k}", keys=TR.KEYS)


def test_draws_are_na_where_s_is_not_positive_and_nan_where_s_is_nan():
    pinned = 0
    for name in EC.CASES:
        for vote in VOTES:
            S = EC.draw_S(name, vote)
            with np.errstate(invalid="ignore"):
                none = ~(S > 0)
            for sample0 in EC.DRAW_SAMPLE0:
                want = EC.draws_all(name, vote, sample0)
                assert np.array_equal(want["h1"] == NA_INTEGER, np.broadcast_to(none[:, None], want["h1"].shape)), (name, vote)
                assert np.array_equal(want["h2"] == NA_INTEGER, want["h1"] == NA_INTEGER)
                assert np.array_equal(np.isnan(want["prob"]), np.broadcast_to(np.isnan(S)[:, None], want["prob"].shape)), (name, vote)
                assert (want["prob"][none & ~np.isnan(S)] == 0).all() and (want["prob"][~none] > 0).all()
        # the contract as written: a row with inf and NaN cells has S = NaN and no draw, although the oracle calls it
        pp, _ = EC.posterior(name, 1)
        mixed = np.isposinf(pp).any(axis=1) & np.isnan(pp).any(axis=1)
        assert np.isnan(EC.draw_S(name, 1)[mixed]).all() and (EC.plain_want(name, 1)["h1"][mixed] != NA_INTEGER).all()
        pinned += int(mixed.sum())
        # an all-inf row: S = inf, no threshold is passed, every draw is the last cell
        allinf = np.isposinf(pp).all(axis=1)
        assert (EC.draws_all(name, 1, 0)["h1"][allinf] == EC.n_hla(name) - 1).all()
    assert pinned >= 5
    # the first n of 64 draws are the call with n draws, and the two numberings draw differently
    for name in ("subnormal-lanes", "mixed-lanes"):
        pp, _ = EC.posterior(name, 1)
        for sample0 in EC.DRAW_SAMPLE0:
            direct = DR.draws_from_postprob(pp, 17, EC.DRAW_SEED, sample0, EC.n_hla(name))
            DR.assert_draws_equal(EC.draws_want(name, 1, 17, sample0), direct, f"{name}, sample0 {sample0}", keys=DR.KEYS)
    a, b = (EC.draws_all("subnormal-lanes", 1, s0)["h1"] for s0 in EC.DRAW_SAMPLE0)
    assert not np.array_equal(a, b) and EC.DRAW_SAMPLE0[1] >> 32 and (EC.DRAW_SAMPLE0[1] + 64) >> 32 != EC.DRAW_SAMPLE0[1] >> 32


def test_groups_partitions_are_what_they_are_called():
    for name in EC.CASES:
        parts = EC.partitions(name)
        n = EC.n_hla(name)
        assert np.array_equal(parts[EC.IDENTITY], np.arange(n)) and (parts[EC.SINGLE] == 0).all()
        assert set(parts[EC.WITH_EMPTY]) == {0, 2} and np.bincount(parts[EC.COARSE]).max() == min(3, n)
        for vote in VOTES:
            want, call = EC.groups_want(name, vote), EC.plain_want(name, vote)
            for key, mine in (("h1", want["g1"][:, 0]), ("h2", want["g2"][:, 0]), ("prob", want["prob"][:, 0]),
                              ("dosage", want["dosage"][:, :n])):
                assert np.array_equal(mine, call[key], equal_nan=True), (name, vote, key)
    # inf + NaN loses, inf + inf wins: the single group's one bin
    want = EC.groups_want("mixed-lanes", 1)
    assert (want["g1"][EC.row_kinds("mixed-lanes") == EC.INF, EC.SINGLE] == NA_INTEGER).all()
    want = EC.groups_want("subnormal-lanes", 1)
    rows = _inf_rows("subnormal-lanes")
    assert (want["g1"][rows, EC.SINGLE] == 0).all() and np.isposinf(want["prob"][rows, EC.SINGLE]).all()


def test_given_sets_move_the_call_and_starve_it():
    moved = starved = 0
    for name in EC.CASES:
        pp, _ = EC.posterior(name, 1)
        call = EC.plain_want(name, 1)
        full = EC.given_want(name, 1, "full")
        for key in ("h1", "h2", "prob", "dosage"):
            assert np.array_equal(full[key], call[key], equal_nan=True), (name, key)
        assert np.array_equal(full["support"], EC.draw_S(name, 1), equal_nan=True), name
        want = EC.given_want(name, 1, "moved")
        for s in np.nonzero(_inf_rows(name))[0]:
            # the consistent cells: all but (c1, c1), (c1, c2), (c2, c2)
            c1, c2 = int(call["h1"][s]), int(call["h2"][s])
            h1, h2 = FR.cell_pairs(EC.n_hla(name))
            left = np.isposinf(pp[s]) & ~(np.isin(h1, (c1, c2)) & np.isin(h2, (c1, c2)))
            if left.any():                                    # the next consistent inf cell
                c = int(left.argmax())
                assert (want["h1"][s], want["h2"][s]) == (h1[c], h2[c]) != (c1, c2) and np.isposinf(want["prob"][s]), (name, s)
                moved += 1
            else:
                assert want["h1"][s] == NA_INTEGER and want["prob"][s] == 0 and np.isnan(want["support"][s]), (name, s)
        want = EC.given_want(name, 1, "nan-only")
        rows = np.isposinf(pp).any(axis=1) & np.isnan(pp).any(axis=1)
        assert (want["h1"][rows] == NA_INTEGER).all() and (want["prob"][rows] == 0).all() and np.isnan(want["support"][rows]).all(), name
        assert (EC.given_sets(name, "nan-only")[rows].sum(axis=2) == 1).all()
        starved += int(rows.sum())
        want = EC.given_want(name, 1, "empty")
        assert (want["h1"] == NA_INTEGER).all() and (want["support"] == 0).all() and (want["dosage"] == 0).all(), name
    assert moved >= 20 and starved >= 5, (moved, starved)
    assert any(_inf_rows(n)[s] and np.isnan(EC.posterior(n, 1)[0][s]).any() and EC.given_want(n, 1, "moved")["h1"][s] != NA_INTEGER
               for n in EC.LANE_CASES[1:] for s in range(200)), "no row with inf and NaN cells has a second inf cell"


def test_family_pedigree_has_the_parent_kinds_and_depths():
    for name in EC.CASES:
        rows, ped = EC.family_case(name)
        depth = FR.depths(ped)                                # (asserts that parents precede their children)
        assert set(rows) == set(range(len(EC.case(name)[1]))) and (ped[:, 0] != ped[:, 1])[ped[:, 0] >= 0].all(), name
        if name not in EC.LANE_CASES:
            assert np.array_equal(depth, (np.arange(len(rows)) % 3 == 2).astype(int)) and np.array_equal(rows, np.arange(len(rows)))
            continue
        kind = EC.row_kinds(name)[rows]
        have = sorted(set(kind))
        pk = np.where(ped >= 0, kind[np.maximum(ped, 0)], EC.OUT)                    # the parents' kinds
        first = (depth <= 1) & (depth[np.maximum(ped, 0)] == 0).all(axis=1)           # children of founders
        for ka in [EC.OUT] + have:
            for kb in [EC.OUT] + have:
                for kc in set(have) & {EC.HEALTHY, EC.INF}:
                    assert (first & (pk[:, 0] == ka) & (pk[:, 1] == kb) & (kind == kc)).any(), (name, ka, kb, kc)
        has = ped >= 0
        same = has & (ped // 64 == np.arange(len(ped))[:, None] // 64)
        assert same.any() and (has & ~same).any(), name
        assert np.count_nonzero(has.any(axis=1) & (np.arange(len(ped)) % 64 < 8)) >= 1
        for with_prior in (True, False):
            S = EC.family_want(name, 1, with_prior)["support"]
            through = np.zeros((3, len(ped)), bool)           # a grandchild through an inf-row parent, a NaN-support one, an inf-support one
            for k in (0, 1):
                p = np.maximum(ped[:, k], 0)
                mid = (ped[:, k] >= 0) & (depth[p] == 1) & (depth == 2)
                through |= np.stack([mid & (kind[p] == EC.INF), mid & np.isnan(S[p]), mid & np.isposinf(S[p])])
            assert through[0].any() and through[1].any(), (name, with_prior)
            if name == "subnormal-lanes":
                assert through[2].any(), with_prior
        # an inf parent (D = inf, S = inf) leaves its child uncalled with NaN support; a NaN-support parent is unknown
        want, none = EC.family_want(name, 1, True), EC.family_want(name, 1, False)
        own = EC.posterior(name, 1)[0][rows]
        for i in np.nonzero(first & (depth == 1))[0]:
            Sp = [want["support"][p] if p >= 0 else 0.0 for p in ped[i]]
            if any(np.isposinf(x) for x in Sp):
                assert want["h1"][i] == NA_INTEGER and np.isnan(want["support"][i]) and np.isnan(want["dosage"][i]).all(), (name, i)
            elif not any(x > 0 for x in Sp):                  # both unknown: the sample's own row
                assert np.array_equal(want["support"][i], np.cumsum(own[i])[-1], equal_nan=True), (name, i)
                assert want["h1"][i] == none["h1"][i]


@pytest.mark.parametrize("name", EC.CASES)
def test_every_finish_reference_runs_on_every_case(name):
    n, nh = len(EC.case(name)[1]), EC.n_hla(name)
    for vote in VOTES:
        for k in EC.TOPK_K:
            assert EC.topk_want(name, vote, k)["prob"].shape == (n, k)
        for d in EC.DRAW_N:
            assert EC.draws_want(name, vote, d, EC.DRAW_SAMPLE0[1])["h1"].shape == (n, d)
        assert EC.groups_want(name, vote)["prob"].shape == (n, 5) and EC.groups_want(name, vote)["dosage"].shape == (n, EC.groups_offsets(name)[-1])
        for which in EC.GIVEN_SETS:
            assert EC.given_want(name, vote, which)["dosage"].shape == (n, nh)
        for with_prior in (True, False):
            assert EC.family_want(name, vote, with_prior)["dosage"].shape == (len(EC.family_case(name)[0]), nh)
