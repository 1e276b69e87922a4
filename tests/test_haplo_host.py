"""hlaHaplotypes without a GPU: the closed-form state count against brute force, the trimming rule on a sample written out
by hand, the summation rule S64 against a hand-written loop, the argument errors raised before the device is touched, the
restatement (tests/haplo_reference.py) on the 200 x 3 synthetic cohort and on phase-unambiguous samples, the declared
symbols."""
import os
import re

import numpy as np
import pytest

import hibag_amd as hb
import haplo_reference as R
from hibag_amd import NA_INTEGER, _lib, haplo
from hibag_amd.topk import HlaTopCalls

NA = NA_INTEGER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def top(locus, ids, h1, h2, prob, n_allele):
    h1, h2, prob = np.asarray(h1, np.int32), np.asarray(h2, np.int32), np.asarray(prob, np.float64)
    return HlaTopCalls(locus, list(ids), h1.shape[1], h1, h2, prob, np.ones(len(ids)), levels=[f"{locus}*{i:02d}" for i in range(n_allele)])


# 1 the state count ----------------------------------------------------------------------------------------------------------
def test_closed_form_state_count_equals_brute_force():
    rng = np.random.default_rng(1)
    seen = set()
    for _ in range(150):
        L = int(rng.integers(2, 5))
        cands = []
        for _l in range(L):
            k = int(rng.integers(1, 4))
            pairs = set()
            while len(pairs) < k:
                a, b = sorted(int(v) for v in rng.integers(0, 3, 2))          # (three alleles: many homozygous pairs)
                pairs.add((a, b))
            cands.append([(a, b, 1.0 / k) for a, b in sorted(pairs)])
        want = R.brute_count(cands)
        assert R.closed_count(cands) == want and len(R.enumerate_states(cands)) == want
        hom =[sum(1 for c in cl if c[0] == c[1]) for cl in cands]
        het = [len(cl) - h for cl, h in zip(cands, hom)]
        assert int(haplo.state_count(hom, het)) == want
        seen.add((L, want))
    assert len(seen) > 20
    assert haplo.state_count([[1, 1], [0, 2]], [[2, 2], [3, 0]]).tolist() == [(25 + 1) // 2, (12 + 0) // 2]


# 2 trimming ---------------------------------------------------------------------------------------------------------------------
def hand_sample():
    """L = 3, k = 4.  Locus 0: (0,1) .50, (0,2) .30, (1,1) .15, (2,2) .05; locus 1: (3,4) .60, (3,3) .30, (4,4) .05, NA;
    locus 2: (5,6) .70, (5,5) .15, (6,6) .15, NA."""
    h1 = np.array([[[0, 0, 1, 2]], [[3, 3, 4, NA]], [[5, 5, 6, NA]]], np.int32)
    h2 = np.array([[[1, 2, 1, 2]], [[4, 3, 4, NA]], [[6, 5, 6, NA]]], np.int32)
    prob = np.array([[[.50, .30, .15, .05]], [[.60, .30, .05, 0.]], [[.70, .15, .15, 0.]]])
    return h1, h2, prob


def test_trimming_rule_by_hand():
    h1, h2, prob = hand_sample()
    cands = R.candidates(h1, h2, prob)[0]
    # untrimmed: (6 * 4 * 4 + 2 * 2 * 2) / 2 = 52 states
    assert R.closed_count(cands) == 52
    # min_prob = 0.1 drops (0, 3) and (1, 2): (5 * 3 * 4 + 1 * 1 * 2) / 2 = 31
    lists, gone = R.trim(cands, 0.1, 4096)
    assert gone == [(0, 3), (1, 2)] and R.closed_count(lists) == 31
    # the cap 12: the smallest p is .15, three times: the highest locus first, there the highest rank: (2, 2), (2, 1), then (0, 2):
    # 31 -> (5 * 3 * 3 + 1) / 2 = 23 -> (5 * 3 * 2 + 0) / 2 = 15 -> (4 * 3 * 2 + 0) / 2 = 12
    lists, gone = R.trim(cands, 0.1, 12)
    assert gone == [(0, 3), (1, 2), (2, 2), (2, 1), (0, 2)] and R.closed_count(lists) == 12
    # the cap 4: then .30 at locus 1 before .30 at locus 0: 12 -> (4 * 2 * 2) / 2 = 8 -> (2 * 2 * 2) / 2 = 4; rank 0 is all that is left
    lists, gone = R.trim(cands, 0.1, 4)
    assert gone[5:] == [(1, 1), (0, 1)] and [len(c) for c in lists] == [1, 1, 1]
    with pytest.raises(ValueError):
        R.trim(cands, 0.1, 3)
    # the package's host half does the same
    for cap, left in ((4096, 31), (12, 12), (4, 4)):
        t1, t2, tp, n_trimmed = haplo.trim_candidates(h1, h2, prob, 0.1, cap)
        want, gone = R.trim(cands, 0.1, cap)
        assert R.candidates(t1, t2, tp)[0] == want and n_trimmed.tolist() == [len(gone)]
        assert (t1[:, 0, 0] == h1[:, 0, 0]).all()                     # rank 0 stays
    with pytest.raises(ValueError, match="'id7'"):
        haplo.trim_candidates(h1, h2, prob, 0.1, 3, ["id7"])
    ids = ["id7"]
    calls = [top("A", ids, h1[0], h2[0], prob[0], 3), top("B", ids, h1[1], h2[1], prob[1], 5), top("C", ids, h1[2], h2[2], prob[2], 7)]
    with pytest.raises(ValueError, match="max_states = 3"):
        hb.hlaHaplotypes(calls, max_states=3, min_prob=0.1, verbose=False)


# 3 S64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129])
def test_s64_against_a_hand_written_loop(n):
    x = np.random.default_rng(n).random(n) * np.float64(10.0) ** np.random.default_rng(n + 1).integers(-8, 8, n)
    lanes = []
    for j in range(64):
        acc = None
        i = j
        while i < n:
            acc = float(x[i]) if acc is None else acc + float(x[i])
            i += 64
        lanes.append(0.0 if acc is None else acc)
    for h in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[j] + lanes[j + h] for j in range(h)]
    assert R.s64(x) == lanes[0] and R._s64_rows(x) == lanes[0]
    if n == 0:
        assert R.s64(x) == 0.0
    if 0 < n <= 16:                                                   # a group of 16 lanes with the butterfly from 8 down
        p = [float(v) for v in x] + [0.0] * (16 - n)
        for h in (8, 4, 2, 1):
            p = [p[j] + p[j + h] for j in range(h)]
        assert p[0] == lanes[0]


def test_s64_in_lane_groups_of_8_and_16():
    rng = np.random.default_rng(9)
    for n in range(1, 17):
        x = rng.random(n)
        for G in (8, 16):
            if n > G:
                continue
            p = list(x) + [0.0] * (G - n)
            h = G // 2
            while h:
                p = [p[j] + p[j + h] for j in range(h)]
                h //= 2
            assert p[0] == R.s64(x), (n, G)


# 4 arguments ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    ids = ["a", "b"]
    one = top("A", ids, [[0], [0]], [[1], [1]], [[1.], [1.]], 2)
    two = top("B", ids, [[0], [0]], [[0], [1]], [[1.], [1.]], 2)
    with pytest.raises(ValueError, match="2 .. 6 loci"):
        hb.hlaHaplotypes([one], verbose=False)
    with pytest.raises(ValueError, match="2 .. 6 loci"):
        hb.hlaHaplotypes([one] * 7, verbose=False)
    with pytest.raises(TypeError):
        hb.hlaHaplotypes(one, verbose=False)
    with pytest.raises(TypeError):
        hb.hlaHaplotypes([one, "B"], verbose=False)
    with pytest.raises(ValueError, match="missing from locus B"):
        hb.hlaHaplotypes([one, top("B", ["a", "c"], [[0], [0]], [[0], [1]], [[1.], [1.]], 2)], verbose=False)
    wide = HlaTopCalls("W", ids, 1, np.zeros((2, 1), np.int32), np.zeros((2, 1), np.int32), np.ones((2, 1)), np.ones(2),
                       levels=[str(i) for i in range(1025)])
    with pytest.raises(ValueError, match="1025 alleles"):
        hb.hlaHaplotypes([one, wide], verbose=False)
    nobody = top("N", ids, [[NA], [0]], [[NA], [0]], [[0.], [0.]], 2)           # an NA rank, a rank with probability 0
    with pytest.raises(ValueError, match="no sample has a candidate"):
        hb.hlaHaplotypes([one, nobody], verbose=False)
    for kw in (dict(max_states=0), dict(max_states=2.5), dict(maxit=0), dict(tol=-1.0), dict(tol=float("nan")), dict(min_prob=2.0)):
        with pytest.raises(ValueError):
            hb.hlaHaplotypes([one, two], verbose=False, **kw)


def test_too_many_states_in_total_is_an_error():
    """Six loci with three heterozygous candidates each: 6^6 / 2 = 23,328 states a sample; 47,000 samples pass 2^30."""
    n = 47000
    ids = list(range(n))
    h1 = np.tile(np.array([0, 0, 1], np.int32), (n, 1))
    h2 = np.tile(np.array([1, 2, 2], np.int32), (n, 1))
    prob = np.tile(np.array([.5, .3, .2]), (n, 1))
    calls = [top(f"L{l}", ids, h1, h2, prob, 3) for l in range(6)]
    with pytest.raises(ValueError, match="2\\^31 - 1 entries"):
        hb.hlaHaplotypes(calls, max_states=32768, verbose=False)


def test_gathering_matches_ids_and_moves_candidates_to_the_front():
    a = top("A", ["x", "y", "z"], [[0, NA], [NA, 1], [1, 0]], [[1, NA], [NA, 0], [1, 0]], [[1., 0.], [0., .4], [.6, 0.]], 2)
    b = hb.HlaAlleleClass(locus="B", sample_id=["z", "x", "y"], allele1=["q", "p", None], allele2=["p", "p", None])
    loci, levels, ids, h1, h2, prob = haplo.gather_candidates({"HLA-A": a, "HLA-B": b})
    assert loci == ["HLA-A", "HLA-B"] and ids == ["x", "y", "z"] and levels[1] == ["p", "q"]
    assert h1[0].tolist() == [[0, NA], [0, NA], [1, NA]] and h2[0].tolist() == [[1, NA], [1, NA], [1, NA]]      # (1, 0) stored as (0, 1)
    assert prob[0].tolist() == [[1., 0.], [.4, 0.], [.6, 0.]]
    assert h1[1].tolist() == [[0, NA], [NA, NA], [0, NA]] and h2[1].tolist() == [[0, NA], [NA, NA], [1, NA]]
    assert prob[1].tolist() == [[1., 0.], [0., 0.], [1., 0.]]


# 5 the restatement ------------------------------------------------------------------------------------------------------------------
def test_joint_calls_improve_on_rank_0():
    """200 samples, 3 loci, a pool of 8 haplotypes, two candidates per locus with an unreliable first rank."""
    truth, h1, h2, prob = R.ld_cohort(200, 3, 2, 8, 12, seed=7)
    before = R.correct_pairs(truth, h1[:, :, 0], h2[:, :, 0])
    r = R.fit(h1, h2, prob)
    after = R.correct_pairs(truth, np.minimum(r["hapA"], r["hapB"]).T, np.maximum(r["hapA"], r["hapB"]).T)
    assert after > before, f"correct per-locus pairs of 600: {before} at rank 0, {after} after the EM"
    assert r["converged"] and r["used"].all() and abs(r["freq"].sum() - 1.0) < 1e-12
    assert r["n_states"].sum() == sum(R.closed_count(c) for c in R.candidates(h1, h2, prob))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_phase_unambiguous_samples_give_exact_counts(seed):
    """k = 1 and at most one heterozygous locus: one state a sample, q = g / g = 1.0, and after any number of iterations
    freq = count / (2 n_used) bit for bit."""
    rng = np.random.default_rng(seed)
    n, L = 40 + 13 * seed, 2 + seed
    a = rng.integers(0, 3, size=(L, n))
    b = a.copy()
    for s in range(n):
        l = int(rng.integers(0, L + 1))
        if l < L:
            b[l, s] = (a[l, s] + 1) % 3
    h1, h2 = np.minimum(a, b)[:, :, None], np.maximum(a, b)[:, :, None]
    shift = (1 << (10 * np.arange(L)))[:, None]
    uniq, count = np.unique(np.concatenate([(a * shift).sum(axis=0), (b * shift).sum(axis=0)]), return_counts=True)
    for maxit in (1, 2, 5):
        r = R.fit(h1, h2, np.ones((L, n, 1)), maxit=maxit, tol=0.0)
        assert np.array_equal(r["keys"], uniq.astype(np.uint64))
        assert r["freq"].tobytes() == (count / (2.0 * n)).tobytes()
        assert (r["prob"] == 1.0).all() and (r["n_states"] == 1).all()


# 6 the library's side ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    for name in ("hibag_hip_haplo_new", "hibag_hip_haplo_free", "hibag_hip_haplo_dims", "hibag_hip_haplo_fit", "hibag_hip_haplo_calls"):
        assert name in _lib.EXPORTS
        assert re.search(r"\b" + name + r"\(", header), name
    assert haplo.MAX_LOCI == int(re.search(r"#define HIBAG_HIP_HAPLO_MAX_LOCI\s+(\d+)", header).group(1))
    assert haplo.MAX_ALLELE == int(re.search(r"#define HIBAG_HIP_HAPLO_MAX_ALLELE\s+(\d+)", header).group(1))
    assert haplo.MAX_K == int(re.search(r"#define HIBAG_HIP_HAPLO_MAX_K\s+(\d+)", header).group(1))
    assert hb.hlaHaplotypes is haplo.hlaHaplotypes and "hlaHaplotypes" in hb.__all__
