"""The edge cases of ``ref_cases.PREDICT_CASES`` are what tests/test_hip_edge_corpus.py needs them to be (CPU, from the
references alone): the subnormal total gives a call with prob = inf, every 64-sample group of ``mixed-lanes`` holds lanes
without a call, with a finite call and with prob = inf side by side -- in the ensemble for every curve size from 4 to 12, and
per classifier for every classifier whose frequencies are scaled down --, a mask heals some poisoned lanes and leaves
others, and a merge meets posterior columns that are NaN in some rows only.  These are conditions on the inputs: where a
recipe misses one, the recipe changes (seed, rate, factor), never the condition."""

import numpy as np
import pytest

import edge_corpus as EC
import ref_cases as RC
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
