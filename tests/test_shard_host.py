"""The host restatement of classifier-sharded prediction (tests/shard_reference.py) pinned on the CPU: against the oracle's
PredictHLA where the order of the additions is the oracle's (one shard; one classifier per shard, whose partial sums are
0 + term, which is exact), within 1e-12 of it where the split moves roundings (2 and 3 shards: a bound on the restatement,
not on the device -- k - 1 additions of non-negative terms differ by a few units of 2^-53), and on planted merged sums, whose
properties are asserted here so that the GPU test of the finish kernels (tests/test_hip_shard.py) cannot become vacuous."""

import numpy as np
import pytest

import shard_reference as R
from conftest import align_geno

NA = R.NA_INTEGER


@pytest.fixture(scope="module")
def hand(oracle):
    model, founders = R.hand_model()
    G = R.hand_samples(model, founders)
    fm = oracle.flatten(model)
    return model, G, fm, oracle.predict(fm, G, vote_method=1)


@pytest.fixture(scope="module")
def hapmap(oracle, hapmap_geno, model_a):
    """The bundled HLA-A model (100 classifiers) on the 60 HapMap CEU samples, 4 % of the genotypes knocked out on top of
    the data's own gaps and sample 7 all missing."""
    G = align_geno(model_a, hapmap_geno, hapmap_geno.sample_id).copy()
    rng = np.random.default_rng(11)
    G[rng.random(G.shape) < 0.04] = NA
    G[7, :] = NA
    fm = oracle.flatten(model_a)
    return model_a, G, fm, oracle.predict(fm, G, vote_method=1)


@pytest.fixture(params=["hand", "hapmap"])
def case(request):
    return request.getfixturevalue(request.param)


def test_the_cases_hold_what_they_are_for(hand, hapmap):
    model, G, fm, want = hand
    widths = sorted({len(c.snpidx) for c in model.classifiers})
    assert len(widths) >= 3 and max(widths) > 32 and len(model.classifiers) == 13
    assert not model.classifiers[R.HAND_EMPTY_AT].haplo
    W = R.classifier_weights(model, G)
    assert (W[:, 5] == 0).all() and want["h1"][5] == NA and want["prob"][5] == 0 and np.isnan(want["matching"][5])
    for c in R.HAND_SKIPPED:                                   # skipped inside a shard: the sample's other classifiers are used
        assert (W[c, 64:67] == 0).all() and (W[c, :64] > 0).sum() > 50
    assert (W[:, 64:67] > 0).sum(axis=0).min() >= 8
    assert (W[R.HAND_GROUP_SKIPPED, 64:128] == 0).all() and (W[R.HAND_GROUP_SKIPPED, 128:] > 0).all()
    used = np.flatnonzero(W[R.HAND_EMPTY_AT] > 0)
    assert used.tolist() == sorted(R.HAND_USE_EMPTY)
    assert np.isnan(want["postprob"][used]).all() and np.isfinite(want["postprob"][np.setdiff1d(np.arange(130), used)]).all()
    assert ((G < 0) | (G > 2)).mean() > 0.02
    model, G, fm, want = hapmap
    assert ((G < 0) | (G > 2)).all(axis=1).tolist() == [i == 7 for i in range(len(G))]
    assert want["h1"][7] == NA and (want["h1"][np.arange(len(G)) != 7] >= 0).all()


def test_one_shard_is_the_oracle_bit_for_bit(oracle, case):
    model, G, fm, want = case
    n, C = G.shape[0], len(model.classifiers)
    full = R.partial_sums(oracle, fm, model, 0, C, G)
    assert full.shape == (fm.n_hla * (fm.n_hla + 1) // 2 + 3, R.n_pad_of(n)) and not full[:, n:].any()
    R.assert_same(R.finish(R.merge([full]), fm.n_hla, n), want, what="one shard")


def test_one_classifier_per_shard_is_the_oracle_bit_for_bit(oracle, case):
    model, G, fm, want = case
    C = len(model.classifiers)
    parts = R.shard_parts(oracle, fm, model, C, G)
    assert len(parts) == C
    R.assert_same(R.finish(R.merge(parts), fm.n_hla, G.shape[0]), want, what="one classifier per shard")
    # and the in-order sum of a run of them is that run's partial sums
    R.assert_same_rows(R.merge(parts[2:7]), R.partial_sums(oracle, fm, model, 2, 7, G), what="classifiers 2..6")


@pytest.mark.parametrize("world", [2, 3])
def test_a_few_shards_keep_the_calls_and_move_the_posteriors_by_roundings(oracle, case, world):
    model, G, fm, want = case
    got = R.finish(R.merge(R.shard_parts(oracle, fm, model, world, G)), fm.n_hla, G.shape[0])
    assert np.array_equal(got["h1"], want["h1"]) and np.array_equal(got["h2"], want["h2"])
    assert np.array_equal(np.isnan(got["postprob"]), np.isnan(want["postprob"]))
    fin = np.isfinite(want["postprob"])
    np.testing.assert_allclose(got["postprob"][fin], want["postprob"][fin], rtol=1e-12, atol=0)


def test_merge_by_rank():
    rng = np.random.default_rng(3)
    parts = [rng.uniform(0, 1, (6, 64)) * 10.0 ** rng.integers(-8, 8) for _ in range(4)]
    R.assert_same_rows(R.merge_by_rank(parts, [0, 0, 0, 0]), ((parts[0] + parts[1]) + parts[2]) + parts[3])
    two = R.merge_by_rank(parts, [0, 0, 1, 1])
    R.assert_same_rows(two, (parts[0] + parts[1]) + (parts[2] + parts[3]))
    R.assert_same_rows(two, (parts[2] + parts[3]) + (parts[0] + parts[1]))           # two addends: either rank's order
    R.assert_same_rows(R.merge_by_rank(parts, [1, 0, 1, 0]), (parts[0] + parts[2]) + (parts[1] + parts[3]))
    assert (two != R.merge(parts)).any()                                              # (the grouping is visible in the bits)
    with pytest.raises(ValueError, match="more than two"):
        R.merge_by_rank(parts, [0, 1, 2, 2])
    with pytest.raises(ValueError):
        R.merge_by_rank(parts, [0, 1])


def test_assert_same_names_key_sample_and_group():
    a = dict(h1=np.zeros(130, np.int32), prob=np.zeros(130))
    b = dict(h1=np.zeros(130, np.int32), prob=np.zeros(130))
    a["prob"][3] = b["prob"][3] = np.nan
    R.assert_same(a, b)
    b["prob"][70] = -0.0                                       # equal as numbers, not in their bits
    with pytest.raises(AssertionError, match=r"prob: 1 samples differ, the first is sample 70 \(group 1\)"):
        R.assert_same(a, b)
    with pytest.raises(AssertionError, match=r"row 2 of 4, sample 65 \(group 1\)"):
        x = np.zeros((4, 128)); y = x.copy(); y[2, 65] = 5e-324
        R.assert_same_rows(x, y)


# ---- the planted merged sums --------------------------------------------------------------------------------------

N_HLA = (1, 2, 5, 6, 16, 17, 23)


def _one(col, n_hla):
    """finish of one planted column; the outputs of its one sample."""
    out = R.finish(col[:, None], n_hla, 1)
    return {k: v[0] for k, v in out.items()}


def _cell(n_hla, h1, h2):
    return h2 + h1 * (2 * n_hla - h1 - 1) // 2


def _block(P, p):
    """(segment, eight-wide block within it or -1 for the cells scanned one by one) of cell p in finish_call."""
    per, segs = R.segments(P)
    g = p // per
    lo, hi = segs[g]
    full = (hi - lo) // 8 * 8
    return g, ((p - lo) // 8 if p - lo < full else -1)


def test_every_planted_property_has_room_somewhere():
    have = {n_hla: set(R.planted_sums(n_hla)[1]) for n_hla in N_HLA}
    every = {f.__name__ for f in R.PLANTS}
    assert have[17] == every and have[23] == every
    assert have[16] == every - {"plant_tie_tail"}             # (nine cells per segment: one is left behind the block of eight)
    assert have[1] == {"plant_zero_weight_positive", "plant_zero_weight_zero", "plant_nan_weight", "plant_nan_only",
                       "plant_subnormal_cells", "plant_subnormal_weight"}
    assert "plant_tie_later_segment" in have[2] and "plant_tie_later_segment" in have[5] and "plant_tie_tail" in have[6]
    # P = 15 is one cell per segment and one segment idle; P = 276 has two full blocks and a tail in a segment
    assert R.segments(15)[0] == 1 and R.segments(15)[1][15] == (15, 15)
    assert R.segments(276)[0] == 18 and R.segments(136)[0] == 9 and R.segments(153)[0] == 10


@pytest.mark.parametrize("n_hla", N_HLA)
def test_planted_columns_have_their_properties(n_hla):
    P = n_hla * (n_hla + 1) // 2
    planted, names = R.planted_sums(n_hla)
    cols = {nm: planted[:, j] for j, nm in enumerate(names)}
    res = {nm: _one(c, n_hla) for nm, c in cols.items()}

    def tie(nm):
        col, r = cols[nm], res[nm]
        at = np.flatnonzero(col[:P] == col[:P].max())
        assert len(at) == 2 and r["h1"] >= 0 and _cell(n_hla, r["h1"], r["h2"]) == at[0]      # the first one is called
        assert r["prob"] == col[at[0]] * (1.0 / col[P])
        return _block(P, at[0]), _block(P, at[1])

    if "plant_tie_same_block" in cols:
        a, b = tie("plant_tie_same_block")
        assert a == b and a[1] >= 0
    if "plant_tie_next_block" in cols:
        a, b = tie("plant_tie_next_block")
        assert a[0] == b[0] and a[1] == 0 and b[1] != 0
        if n_hla == 23:
            assert b[1] == 1                                   # a second eight-wide block of the same segment
    if "plant_tie_tail" in cols:
        a, b = tie("plant_tie_tail")
        assert a == b and a[1] == -1
    if "plant_tie_later_segment" in cols:
        a, b = tie("plant_tie_later_segment")
        assert a[0] < b[0]
    if "plant_scaled_tie" in cols:
        col, r = cols["plant_scaled_tie"], res["plant_scaled_tie"]
        ff = 1.0 / col[P]
        assert col[0] < col[1] and col[0] * ff == col[1] * ff and np.nextafter(col[0], np.inf) == col[1]
        assert col[:P].argmax() == 1 and (r["h1"], r["h2"]) == (0, 0) and r["prob"] == col[0] * ff
        assert r["postprob"][0] == r["postprob"][1]
    col, r = cols["plant_zero_weight_positive"], res["plant_zero_weight_positive"]
    assert col[P] == 0 and (col[:P] > 0).all() and np.array_equal(r["postprob"], col[:P])
    assert r["h1"] >= 0 and r["prob"] == col[:P].max() and np.isinf(r["matching"])
    r = res["plant_zero_weight_zero"]
    assert r["h1"] == NA and r["h2"] == NA and r["prob"] == 0.0 and np.isnan(r["matching"])
    assert not r["postprob"].any() and not r["dosage"].any()
    col, r = cols["plant_nan_weight"], res["plant_nan_weight"]
    assert np.isnan(col[P]) and np.isfinite(col[:P]).all()
    assert r["h1"] == NA and np.isnan(r["prob"]) and np.isnan(r["dosage"]).all() and np.isnan(r["postprob"]).all()
    assert r["matching"] == col[P + 1] / col[P + 2]
    if "plant_nan_before_max" in cols:
        col, r = cols["plant_nan_before_max"], res["plant_nan_before_max"]
        assert np.isnan(col[0]) and np.nanargmax(col[:P]) == P - 1
        assert _cell(n_hla, r["h1"], r["h2"]) == P - 1 and r["prob"] == 3.0 * (1.0 / col[P])
        assert np.isnan(r["postprob"][0]) and np.isnan(r["dosage"][0]) and np.isfinite(r["postprob"][1:]).all()
    col, r = cols["plant_nan_only"], res["plant_nan_only"]
    assert np.isnan(col[:P]).sum() == 1 and np.nansum(col[:P]) == 0
    assert r["h1"] == NA and r["prob"] == 0.0 and np.isnan(r["postprob"]).sum() == 1
    if "plant_inf_twice" in cols:
        col, r = cols["plant_inf_twice"], res["plant_inf_twice"]
        at = np.flatnonzero(np.isinf(col[:P]))
        assert len(at) == 2 and _cell(n_hla, r["h1"], r["h2"]) == at[0] and r["prob"] == np.inf
    col, r = cols["plant_subnormal_cells"], res["plant_subnormal_cells"]
    assert (col[:P] > 0).all() and (col[:P] < 2.3e-308).all() and not r["postprob"].any()
    assert r["h1"] == NA and r["prob"] == 0.0 and not r["dosage"].any()
    col, r = cols["plant_subnormal_weight"], res["plant_subnormal_weight"]
    with np.errstate(over="ignore"):
        assert 0 < col[P] < 2.3e-308 and np.isinf(1.0 / col[P])
    assert (r["h1"], r["h2"]) == (0, 0) and r["prob"] == np.inf and np.isinf(r["postprob"]).all()


@pytest.mark.parametrize("n", [1, 64, 130])
def test_synthetic_sums_carry_the_planted_columns_in_every_group(n):
    for n_hla in N_HLA:
        P = n_hla * (n_hla + 1) // 2
        sums, where = R.synthetic_merged(n_hla, n)
        planted, names = R.planted_sums(n_hla)
        assert sums.shape == (P + 3, R.n_pad_of(n)) and sums.dtype == np.float64
        for s, nm in where.items():
            assert s < n and np.array_equal(sums[:, s], planted[:, names.index(nm)], equal_nan=True)
        rest = np.setdiff1d(np.arange(n), list(where))
        assert (sums[:P + 1, rest] > 0).all() and np.isfinite(sums[:, rest]).all()
        if n == 1:
            assert where == {0: names[0]}
        else:
            assert len(rest) >= n // 4
            for g in range((n + 63) // 64):
                assert any(s // 64 == g for s in where) and any(s // 64 == g for s in rest)
            assert {where[s] for s in where if s < 64} == set(names)
            # finish treats a sample alone as it treats it among the others
            all_at_once = R.finish(sums, n_hla, n)
            s = max(where)
            R.assert_same({k: v[s:s + 1] for k, v in all_at_once.items()}, R.finish(sums[:, s:s + 1], n_hla, 1))


def test_the_hand_built_case_tells_a_wrong_merge_or_finish_apart(oracle, hand):
    """What the GPU comparisons rest on: on this case another order of the shards, or a finish that divides by the weight
    sum where the kernels multiply by its reciprocal, changes bits."""
    model, G, fm, want = hand
    for world in (3, 5):
        parts = R.shard_parts(oracle, fm, model, world, G)
        a, b = R.merge(parts), R.merge(parts[::-1])
        assert (a[:15, :130] != b[:15, :130]).sum() > 100
        with pytest.raises(AssertionError):
            R.assert_same(R.finish(b, 5, 130), R.finish(a, 5, 130))
    full = R.partial_sums(oracle, fm, model, 0, 13, G)
    ok = full[15, :130] > 0
    divided = full[:15, :130][:, ok] / full[15, :130][ok]
    assert (divided.T != R.finish(full, 5, 130)["postprob"][ok]).sum() > 100
