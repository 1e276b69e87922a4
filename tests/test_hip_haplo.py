"""hlaHaplotypes on the GPU: frequencies, keys, iteration count, delta, totals, the called haplotypes and their posteriors
equal the restatement (tests/haplo_reference.py: DESIGN.md section 29 in plain Python) bit for bit -- every operation is an
IEEE FP64 add, multiply or divide in a defined order, so there is no tolerance -- on a cohort written out by hand, on a
synthetic cohort with linkage disequilibrium and every kind of input, at the seams of the summation rule (state counts and
list lengths around 8, 16, 64 and 128), and in the corners: exact counting without the restatement, key packing at six loci,
maxit, tol = 0, a sample of likelihood 0, repeated fits, one sample."""
import numpy as np
import pytest

import hibag_amd as hb
import haplo_reference as R
from hibag_amd import NA_INTEGER, _lib, haplo
from hibag_amd.topk import HlaTopCalls

pytestmark = pytest.mark.gpu

NA = NA_INTEGER


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def levels(l, n_allele):
    return [f"L{l}*{i:04d}" for i in range(n_allele)]


def make_calls(h1, h2, prob, n_allele, as_class=()):
    """The arrays [L][n][k] as hlaHaplotypes takes them -- an HlaTopCalls per locus, for the loci of `as_class` an
    HlaAlleleClass of rank 0 -- and the arrays the restatement gets for the same input."""
    L, n, k = h1.shape
    ids = [f"s{i}" for i in range(n)]
    calls = {}
    r1, r2, rp = h1.copy(), h2.copy(), prob.copy()
    for l in range(L):
        na = n_allele[l] if isinstance(n_allele, (list, tuple)) else n_allele
        if l in as_class:
            calls[f"L{l}"] = hb.HlaAlleleClass(locus=f"L{l}", sample_id=list(ids), h1=h1[l, :, 0].copy(), h2=h2[l, :, 0].copy(),
                                               levels=levels(l, na), prob=prob[l, :, 0].copy())
            r1[l, :, 1:], r2[l, :, 1:], rp[l, :, 1:] = NA, NA, 0.0
            rp[l, :, 0] = 1.0
        else:
            calls[f"L{l}"] = HlaTopCalls(f"L{l}", list(ids), k, h1[l], h2[l], prob[l], np.ones(n), levels=levels(l, na))
    return calls, (r1, r2, rp)


def assert_same(res, ref, what=""):
    """Every number of the result against the restatement's, bit for bit."""
    order = np.argsort(res.keys, kind="stable")
    assert np.array_equal(res.keys[order], ref["keys"]), what
    bad = np.flatnonzero(bits(res.freq[order]) != bits(ref["freq"]))
    assert bad.size == 0, f"{what}: {bad.size} of {len(ref['freq'])} frequencies differ, the first at {bad[0]}: " \
                          f"{res.freq[order][bad[0]]!r} vs {ref['freq'][bad[0]]!r}"
    assert res.n_iter == ref["n_iter"], (what, res.n_iter, ref["n_iter"])
    assert bits(res.delta) == bits(ref["delta"]), (what, res.delta, ref["delta"])
    assert res.converged == ref["converged"] and res.n_zero == ref["n_zero"], what
    assert np.array_equal(res.used, ref["used"]) and np.array_equal(res.n_states, ref["n_states"]), what
    assert np.array_equal(res.n_trimmed, ref["n_trimmed"]), what
    assert np.array_equal(bits(res.total), bits(ref["total"])), what
    assert np.array_equal(bits(res.prob), bits(ref["prob"])), what
    assert np.array_equal(res.h1, ref["hapA"]) and np.array_equal(res.h2, ref["hapB"]), what
    assert res.loglik == ref["loglik"], what
    # the result's own order: frequency descending, equal frequencies by ascending key
    f, k = res.freq, res.keys
    assert np.all((f[:-1] > f[1:]) | ((f[:-1] == f[1:]) & (k[:-1] < k[1:]))), what
    assert np.array_equal(res.haplotypes, haplo.decode_keys(res.keys, len(res.loci))), what


def both(h1, h2, prob, n_allele, as_class=(), **kw):
    calls, arrays = make_calls(h1, h2, prob, n_allele, as_class)
    res = hb.hlaHaplotypes(calls, verbose=False, **kw)
    ref = R.fit(*arrays, **kw)
    return res, ref


# 1 by hand ---------------------------------------------------------------------------------------------------------------
def hand_cohort():
    h1 = np.array([[[0, 0], [0, NA], [0, 1]], [[2, 2], [2, NA], [3, NA]]], np.int32)
    h2 = np.array([[[1, 0], [0, NA], [1, 1]], [[3, 2], [2, NA], [3, NA]]], np.int32)
    prob = np.array([[[.7, .3], [1., 0.], [.9, .1]], [[.6, .4], [1., 0.], [1., 0.]]])
    return h1, h2, prob


def test_three_samples_by_hand():
    h1, h2, prob = hand_cohort()
    res, ref = both(h1, h2, prob, 4)
    # sample 0: (01, 23) two phases, (01, 22), (00, 23), (00, 22); sample 1: one state; sample 2: (01, 33), (11, 33)
    assert res.n_states.tolist() == [5, 1, 2]
    # the haplotypes (locus 0, locus 1): (0, 2), (1, 2), (0, 3), (1, 3); key = a0 + (a1 << 10)
    assert sorted(res.keys.tolist()) == [2048, 2049, 3072, 3073]
    assert ref["list_lengths"].tolist() == [7, 2, 3, 4]
    assert_same(res, ref, "by hand")
    assert res.names(0) == "L0*0000~L1*0002" and abs(res.freq.sum() - 1) < 1e-12
    # one iteration, every operation written out: f = 1/4, g = (wc f) f, tot by S64 (h = 4, 2, 1 for 5 states), f' = S64(q) / 6
    one, _ = both(h1, h2, prob, 4, maxit=1)
    f = 1.0 / 4
    wc = [(.7 * .6) * 2.0, (.7 * .6) * 2.0, (.7 * .4) * 2.0, (.3 * .6) * 2.0, (.3 * .4) * 1.0]
    g = [(w * f) * f for w in wc]
    tot0 = ((g[0] + g[4]) + g[2]) + (g[1] + g[3])
    q0 = [v / tot0 for v in g]
    g2 = [((.9 * 1.) * 2.0 * f) * f, ((.1 * 1.) * 1.0 * f) * f]
    q2 = [v / (g2[0] + g2[1]) for v in g2]
    # lists in entry order: (0,2): s0 A, s2 A, s3 A, s4 A, s4 B, and sample 1's state twice; (1,2): s1 B, s2 B; (0,3): s1 A, s3 B,
    # sample 2's first A; (1,3): s0 B, sample 2: first B, second A and B
    x = [q0[0], q0[2], q0[3], q0[4], q0[4], 1.0, 1.0]
    f02 = (((x[0] + x[4]) + (x[2] + x[6])) + ((x[1] + x[5]) + x[3])) / 6.0
    f13 = ((q0[0] + q2[1]) + (q2[0] + q2[1])) / 6.0
    by_key = dict(zip(one.keys.tolist(), one.freq.tolist()))
    assert by_key[2048] == f02 and by_key[3073] == f13
    assert one.n_iter == 1 and not one.converged


# 2 the synthetic cohort ----------------------------------------------------------------------------------------------------
def test_ld_cohort_with_every_kind_of_input():
    truth, h1, h2, prob = R.ld_cohort(130, 3, 3, 8, 12, seed=11)
    h1[0, 3::7, 2] = NA; h2[0, 3::7, 2] = NA; prob[0, 3::7, 2] = 0.0          # NA ranks
    h1[1, 4::9, 1] = NA; h2[1, 4::9, 1] = NA; prob[1, 4::9, 1] = 0.0          # an NA rank in the middle
    h1[1, 5, :] = NA; h2[1, 5, :] = NA; prob[1, 5, :] = 0.0                   # a sample with an NA locus
    for l in range(3):                                                        # an all-homozygous sample
        h1[l, 7, :], h2[l, 7, :], prob[l, 7, :] = [l + 1, NA, NA], [l + 1, NA, NA], [1.0, 0.0, 0.0]
    res, ref = both(h1, h2, prob, 12, as_class=(2,))
    assert not res.used[5] and res.used.sum() == 129 and res.h1[5, 0] == NA and np.isnan(res.prob[5])
    assert res.n_states[7] == 1 and res.n_iter > 8                            # (more than one batch of iterations)
    assert_same(res, ref, "LD cohort")
    assert np.array_equal(res.locus_calls("L1").h1[res.used], np.minimum(ref["hapA"], ref["hapB"])[res.used, 1])
    assert res.n_changed.shape == (3,) and res.n_changed[2] == 0              # a certain locus never changes


# 3 the seams of S64 --------------------------------------------------------------------------------------------------------
LIST_LENGTHS = (1, 2, 8, 9, 16, 17, 63, 64, 65, 129)
STATE_COUNTS = (1, 63, 64, 65, 648)


def seam_cohort():
    """L = 4, k = 5.  Samples 0 .. 4 have 1, 63, 64, 65 and 648 states (alleles from 40 up at locus 0); then, for every
    length m of LIST_LENGTHS, m samples heterozygous at locus 0 alone between the allele 2 i (in no other sample) and the
    filler 2 i + 1, with two homozygous candidates of random weight at locus 1: the haplotype (2 i, 0, 0, 0) has m entries."""
    rng = np.random.default_rng(5)
    rows = []

    def sample(*loci):
        rows.append([list(c) + [(NA, NA, 0.0)] * (5 - len(c)) for c in loci])

    def weights(n):
        p = rng.dirichlet(np.full(n, 3.0))
        return np.sort(p)[::-1]

    def cands(pairs):
        return [(a, b, p) for (a, b), p in zip(pairs, weights(len(pairs)))]

    one = [(0, 0, 1.0)]
    het = [(40, 41), (40, 42), (41, 43), (42, 43), (44, 45)]
    hom = [(40, 40), (41, 41), (42, 42), (43, 43), (44, 44)]
    sample([(40, 40, 1.0)], one, one, one)                                                   # 1
    sample(cands([hom[0]] + het[:2]), cands([(1, 1), (1, 2), (2, 3)]), cands([(3, 3), (3, 4), (4, 5)]), one)   # (5^3 + 1) / 2 = 63
    sample(cands(het[:1]), cands([(1, 2), (2, 3), (3, 4), (4, 5)]), cands([(1, 2), (2, 3), (3, 4), (4, 5)]), one)   # 2 * 8 * 8 / 2 = 64
    sample(cands(hom), cands([(1, 1), (1, 2), (2, 3)]), cands([(3, 3), (3, 4), (4, 5)]), one)      # (5^3 + 5) / 2 = 65
    sample(cands(het[:3]), cands([(1, 2), (2, 3), (3, 4)]), cands([(1, 2), (2, 3), (3, 4)]), cands([(0, 1), (1, 2), (2, 3)]))   # 6^4 / 2 = 648
    for i, m in enumerate(LIST_LENGTHS):
        for _ in range(m):
            sample([(2 * i, 2 * i + 1, 1.0)], cands([(0, 0), (6, 6)]), one, one)
    a = np.array(rows, dtype=object)                                  # [n][L][k][3]
    h1 = np.ascontiguousarray(a[..., 0].astype(np.int32).transpose(1, 0, 2))
    h2 = np.ascontiguousarray(a[..., 1].astype(np.int32).transpose(1, 0, 2))
    prob = np.ascontiguousarray(a[..., 2].astype(np.float64).transpose(1, 0, 2))
    return h1, h2, prob


def test_seams_of_the_summation_rule():
    h1, h2, prob = seam_cohort()
    res, ref = both(h1, h2, prob, 48, min_prob=0.0)
    assert res.n_states[:5].tolist() == list(STATE_COUNTS)
    for i, m in enumerate(LIST_LENGTHS):                              # the haplotype (2 i, 0, 0, 0) has the key 2 i
        at = int(np.flatnonzero(ref["keys"] == 2 * i)[0])
        assert ref["list_lengths"][at] == m, (m, ref["list_lengths"][at])
    assert_same(res, ref, "seams")


# 4 exact counting, without the restatement ------------------------------------------------------------------------------------
def test_phase_unambiguous_samples_give_exact_counts():
    rng = np.random.default_rng(3)
    n, L = 57, 3
    a = rng.integers(0, 4, size=(L, n))
    b = a.copy()
    het_at = rng.integers(0, L + 1, n)                                # (L: no heterozygous locus)
    for s in range(n):
        if het_at[s] < L:
            b[het_at[s], s] = (a[het_at[s], s] + 1 + rng.integers(0, 3)) % 4
    h1, h2 = np.minimum(a, b)[:, :, None].astype(np.int32), np.maximum(a, b)[:, :, None].astype(np.int32)
    calls, _ = make_calls(h1, h2, np.ones((L, n, 1)), 4, as_class=(0, 1, 2))
    keys = np.concatenate([(a * (1 << (10 * np.arange(L)))[:, None]).sum(axis=0), (b * (1 << (10 * np.arange(L)))[:, None]).sum(axis=0)])
    uniq, count = np.unique(keys, return_counts=True)
    for kw in (dict(maxit=1), dict(maxit=2), dict(maxit=7, tol=0.0)):
        res = hb.hlaHaplotypes(calls, verbose=False, **kw)
        order = np.argsort(res.keys)
        assert np.array_equal(res.keys[order], uniq.astype(np.uint64))
        assert np.array_equal(bits(res.freq[order]), bits(count / (2.0 * n))), kw
        assert (res.n_states == 1).all() and (res.prob == 1.0).all()
    assert res.n_iter == 2 and res.converged and res.delta == 0.0     # the second iteration changes nothing: tol = 0 is met


# 5 key packing --------------------------------------------------------------------------------------------------------------
def test_six_loci_and_allele_1023_decode_back():
    h1 = np.zeros((6, 2, 1), np.int32)
    h1[5] = 1023
    calls, arrays = make_calls(h1, h1.copy(), np.ones((6, 2, 1)), [1, 1, 1, 1, 1, 1024])
    res = hb.hlaHaplotypes(calls, verbose=False)
    assert res.keys.tolist() == [1023 << 50] and res.haplotypes.tolist() == [[0, 0, 0, 0, 0, 1023]]
    assert res.freq.tolist() == [1.0] and res.h1.tolist() == [[0, 0, 0, 0, 0, 1023]] * 2
    assert res.names(0) == "L0*0000~L1*0000~L2*0000~L3*0000~L4*0000~L5*1023"
    assert_same(res, R.fit(*arrays), "six loci")


# 6 the stopping rule --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cohort():
    _, h1, h2, prob = R.ld_cohort(40, 2, 2, 5, 6, seed=2)
    return h1, h2, prob


@pytest.mark.parametrize("kw", [dict(maxit=1), dict(maxit=3, tol=1e-300), dict(maxit=9, tol=1e-300), dict(tol=0.0), dict(tol=1e-3)],
                         ids=["maxit1", "maxit3", "maxit9", "tol0", "tol1e-3"])
def test_stopping_rule(small_cohort, kw):
    res, ref = both(*small_cohort, 6, **kw)
    assert_same(res, ref, str(kw))
    if "maxit" in kw:
        assert res.n_iter == kw["maxit"] and not res.converged


# 7 a sample of likelihood 0 ---------------------------------------------------------------------------------------------------
def test_a_sample_whose_total_is_zero(small_cohort):
    h1, h2, prob = (a.copy() for a in small_cohort)
    h1[:, 3, 1] = NA; h2[:, 3, 1] = NA; prob[:, 3, 1] = 0.0
    prob[:, 3, 0] = 5e-324                                            # the product of two such weights is 0
    res, ref = both(h1, h2, prob, 6)
    assert res.n_zero == 1 and res.used[3] and res.total[3] == 0.0 and res.prob[3] == 0.0
    assert not np.isnan(res.freq).any() and not np.isnan(res.prob[res.used]).any() and np.isfinite(res.loglik)
    assert_same(res, ref, "zero total")


# 8 handles ------------------------------------------------------------------------------------------------------------------
def test_two_fits_on_one_handle_are_identical(small_cohort):
    h1, h2, prob = small_cohort
    with haplo._DeviceHaplo(h1, h2, prob, 4096) as dev:
        a, ca = dev.fit(200, 1e-8), dev.calls()
        dev.fit(2, 0.0)
        b, cb = dev.fit(200, 1e-8), dev.calls()
    for k in ("freq", "keys"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["n_iter"], a["delta"], a["n_zero"]) == (b["n_iter"], b["delta"], b["n_zero"])
    for k in ca:
        assert ca[k].tobytes() == cb[k].tobytes(), k


def test_one_sample():
    h1, h2, prob = (a[:, :1].copy() for a in hand_cohort())
    res, ref = both(h1, h2, prob, 4)
    assert res.n_used == 1 and res.n_states.tolist() == [5]
    assert_same(res, ref, "one sample")


def test_the_library_rejects_what_the_host_rejects():
    z, p = np.zeros((2, 1, 1), np.int32), np.ones((2, 1, 1))
    for args in ((np.zeros((1, 1, 1), np.int32), np.zeros((1, 1, 1), np.int32), np.ones((1, 1, 1)), 16),      # one locus
                 (np.zeros((7, 1, 1), np.int32), np.zeros((7, 1, 1), np.int32), np.ones((7, 1, 1)), 16),      # seven
                 (z + 1024, z + 1024, p, 16),                                                               # allele index 1024
                 (np.full((2, 1, 1), NA, np.int32), np.full((2, 1, 1), NA, np.int32), p, 16),                 # nobody used
                 (np.array([[[0, 0]], [[0, 0]]], np.int32), np.array([[[1, 2]], [[1, 2]]], np.int32), np.ones((2, 1, 2)), 7)):   # 8 states
        with pytest.raises(_lib.HibagHipError) as e:
            haplo._DeviceHaplo(*args)
        assert "hibag_hip_haplo_new" in str(e.value)
