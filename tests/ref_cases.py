"""Inputs shared by tests/test_ref_pin.py (the oracle against the compiled reference, CPU) and
tests/test_hip_ref_host.py (the compiled reference as the host of the plugin table, GPU), and the comparisons both use.
Everything is compared as bits: a float's byte pattern, not its value."""

import numpy as np

from hibag_amd import NA_INTEGER, synth
from hibag_amd.model import Classifier, HlaAttrBagObj

KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")

# every SNP count at which a packed word fills up or a second one begins, and a few inside
WIDTHS = [1, 5, 24, 31, 32, 33, 40, 63, 64, 65, 100, 127, 128]


def assert_same_bits(got, want, what=""):
    """All six outputs of PredictHLA, byte for byte."""
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if a.tobytes() != b.tobytes():
            ua, ub = a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32), b.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
            bad = np.argwhere(ua != ub)
            i = tuple(bad[0])
            raise AssertionError(f"{what}: '{k}': {len(bad)} entries differ as bits, first at {i}: {a[i]!r} ({int(ua[i]):#x}) "
                                 f"against {b[i]!r} ({int(ub[i]):#x})")


def width_model(n_samp=60, widths=WIDTHS, seed=77):
    """One classifier per SNP count of ``widths``; ``n_samp`` samples drawn from the model, 5 % missing, sample 3 all NA."""
    model, founders, af = synth.make_model("hla-a-small", seed=seed, n_classifier=len(widths), n_snp=160,
                                           snp_counts=widths, wide_classifier=False)
    G, _ = synth.make_samples(founders, af, n_samp, seed=seed + 1, miss=0.05)
    G[3, :] = NA_INTEGER
    return model, G


def no_haplotype_model():
    """A classifier with SNPs and no haplotype (total 0 where its SNPs are typed), one with neither, between two usual ones."""
    model, founders, af = synth.make_model("hla-a-small", seed=5, n_classifier=2, n_snp=40, wide_classifier=False)
    none = Classifier(np.array([3, 9, 11], np.int32), np.zeros(0), np.zeros(0, np.int32), [])
    nothing = Classifier(np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32), [])
    model.classifiers = [model.classifiers[0], none, nothing, model.classifiers[1]]
    G, _ = synth.make_samples(founders, af, 12, seed=6, miss=0.05)
    G[2, [3, 9, 11]] = NA_INTEGER                     # the haplotype-less classifier has weight 0 for this sample
    G[4, :] = NA_INTEGER
    return model, G


def zero_frequency_model():
    """Haplotypes of frequency 0: single ones, a whole allele's, and a classifier whose every frequency is 0."""
    model, founders, af = synth.make_model("hla-a-small", seed=9, n_classifier=4, n_snp=50, wide_classifier=False)
    c0, c1, c2, _ = model.classifiers
    c0.freq = c0.freq.copy(); c0.freq[::3] = 0.0
    c1.freq = c1.freq.copy(); c1.freq[c1.hla == c1.hla[len(c1.hla) // 2]] = 0.0
    c2.freq = np.zeros_like(c2.freq)
    G, _ = synth.make_samples(founders, af, 16, seed=10, miss=0.03)
    return model, G


def underflow_model():
    """tests/test_hip_parity.py::test_underflow_gives_nan_like_the_reference: a classifier whose every pair is >= 65
    mismatches away has total 0, 1 / total = inf and 0 * inf = NaN (src/LibHLA.cpp:1826-1828)."""
    k = 100
    far = Classifier(np.arange(k), [0.5, 0.5], [0, 1], ["1" * k, "1" * k])
    near = Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    model = HlaAttrBagObj(0, k, ["a", "b", "c"], [near, far])
    G = np.zeros((3, k), np.int32)
    G[1, 40:] = NA_INTEGER
    G[2, :] = NA_INTEGER
    return model, G


def mirrored_model():
    """Two alleles with the same haplotypes and frequencies: bit-equal cells tied at the maximum (tests/test_hip_topk.py)."""
    from test_hip_topk import mirrored_case
    return mirrored_case()


def odd_values_model():
    """-1, 3 and NA in the genotypes: each is missing (TGenotype::IntToSNP, src/LibHLA.cpp:662-706; the weights, :2427)."""
    model, founders, af = synth.make_model("hla-a-small", seed=13, n_classifier=6, n_snp=60, wide_classifier=False)
    G, _ = synth.make_samples(founders, af, 20, seed=14, miss=0.0)
    rng = np.random.default_rng(15)
    r = rng.random(G.shape)
    G[r < 0.04] = -1
    G[(r >= 0.04) & (r < 0.08)] = 3
    G[(r >= 0.08) & (r < 0.12)] = NA_INTEGER
    G[5, :] = 3
    G[6, :] = -1
    G[7, ::2] = 7
    return model, G


def subnormal_model():
    """A total that is positive and below 1 / DBL_MAX: 1 / total = inf, so the positive cells become inf and the empty ones
    0 * inf = NaN, and the reference still makes a call, with prob = inf (the first inf cell; src/LibHLA.cpp:1826-1828).
    Every pair of ``sub`` is 62 to 64 mismatches from sample 0: its total is a few 1e-310.  Sample 1 (one SNP fewer) and
    sample 3 (four mismatches fewer) have normal totals, sample 2 types nothing."""
    k = 32
    near = Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    sub = Classifier(np.arange(k), [0.4, 0.2, 0.2, 0.2], [0, 0, 1, 2],
                     ["1" * k, "0" + "1" * (k - 1), "1" + "0" + "1" * (k - 2), "1" * k])
    model = HlaAttrBagObj(0, k, ["a", "b", "c"], [near, sub])
    G = np.zeros((4, k), np.int32)
    G[1, k - 1] = NA_INTEGER
    G[2, :] = NA_INTEGER
    G[3, :2] = 2
    return model, G


def subnormal_lanes_model(n_samp=72):
    """The four samples of ``subnormal_model`` dealt over 72 lanes in a seeded order, so that a 64-sample group holds finite,
    inf, NaN-matching lanes side by side (and the group of eight that follows it too).  The inf lanes' posterior is inf in
    every cell and NaN in none -- every pair of ``sub`` exists and stays positive --, which is what a merge with a second
    model needs to normalise a column to NaN in some rows and 0 in others."""
    model, four = subnormal_model()
    kind = np.random.default_rng(5).integers(0, 4, n_samp)
    kind[:4] = np.arange(4)
    return model, np.ascontiguousarray(four[kind])


MIXED_COUNTS = [12, 113, 18, 40, 24, 30, 31, 32, 56, 84, 100, 120, 128, 20]
MIXED_SCALE = 1e-140
# which classifiers' haplotype frequencies are scaled down, by what, and the error rate at the noisy end of a 64-sample group
MIXED_ENSEMBLE = {"scaled": {3: MIXED_SCALE, 12: MIXED_SCALE}, "rate": 0.25}
MIXED_PER_CLASSIFIER = {"scaled": {0: 1e-150, 1: MIXED_SCALE, 3: MIXED_SCALE, 6: MIXED_SCALE, 7: MIXED_SCALE, 9: MIXED_SCALE},
                        "rate": 0.5}
MIXED_ALL_MISSING = 7


def mixed_lanes_model(recipe=MIXED_ENSEMBLE, n_samp=200):
    """Healthy, inf, NaN and inactive lanes inside one 64-sample group.  The engine-mix model of the curve and out-of-bag
    tests (one-step and multi-step matrix engine, int8, VALU) on 200 samples: three full groups and one of eight.  Sample s
    gets uniform random genotype errors at rate (s % 64) / 64 * rate, so every group runs from clean to noisy, and the
    haplotype frequencies of the ``scaled`` classifiers are multiplied by 1e-140 or less (tests/test_hip_chunks.py::
    underflow_model): a sample a few mismatches from its best pair has a subnormal total there (1 / total = inf: inf in its
    positive cells, NaN in its empty ones, and a call with prob = inf -- the first inf cell), one further away has total 0
    (NaN in every cell: no call).  Sample 7 types nothing.  ``MIXED_ENSEMBLE`` ("mixed-lanes") is for the entries that sum
    over classifiers, ``MIXED_PER_CLASSIFIER`` ("mixed-lanes-each") for the ones that evaluate each classifier on its own: a
    scaled classifier on every pick kernel, and 1e-150 for the 12-SNP one, which 1e-140 leaves nearly without such lanes."""
    model, founders, af = synth.make_model("hla-b", seed=7, n_snp=160, n_classifier=len(MIXED_COUNTS), snp_counts=MIXED_COUNTS)
    G, _ = synth.make_samples(founders, af, n_samp, seed=8)
    rng = np.random.default_rng(29)
    rate = (np.arange(n_samp) % 64) / 64.0 * recipe["rate"]
    wrong = rng.random(G.shape) < rate[:, None]
    G = np.where(wrong & (G != NA_INTEGER), rng.integers(0, 3, G.shape), G).astype(np.int32)
    G[MIXED_ALL_MISSING, :] = NA_INTEGER
    for c, factor in recipe["scaled"].items():
        model.classifiers[c].freq = np.asarray(model.classifiers[c].freq, np.float64) * factor
    return model, np.ascontiguousarray(G)


def mixed_lanes_per_classifier():
    """``mixed_lanes_model`` with the ``MIXED_PER_CLASSIFIER`` recipe."""
    return mixed_lanes_model(MIXED_PER_CLASSIFIER)


PREDICT_CASES = {"widths": width_model, "no-haplotypes": no_haplotype_model, "zero-frequency": zero_frequency_model,
                 "underflow": underflow_model, "mirrored": mirrored_model, "odd-values": odd_values_model,
                 "subnormal": subnormal_model, "subnormal-lanes": subnormal_lanes_model, "mixed-lanes": mixed_lanes_model,
                 "mixed-lanes-each": mixed_lanes_per_classifier}


def lane_kinds(h1, prob):
    """(no call, finite call, call with prob = +inf) as boolean arrays."""
    h1, prob = np.asarray(h1), np.asarray(prob)
    na = h1 == NA_INTEGER
    return na, ~na & np.isfinite(prob), ~na & np.isposinf(prob)


def training_cohort(n_samp=80, n_snp=60, n_hla=7, seed=41):
    """80 samples x 60 SNPs: each allele has three haplotype variants a few sites apart, genotypes are sums of two of them
    with 4 % errors and 3 % missing.  Variants and errors keep the greedy search going for several SNPs and leave the
    out-of-bag accuracy below 1."""
    rng = np.random.default_rng(seed)
    base = (rng.random((n_hla, n_snp)) < 0.45).astype(np.int32)
    for a in range(1, n_hla, 2):                       # pairs of alleles that differ at two SNPs only
        base[a] = base[a - 1]
        base[a, rng.choice(n_snp, 2, replace=False)] ^= 1
    var = np.repeat(base[:, None, :], 3, axis=1)
    for a in range(n_hla):
        for v in range(1, 3):
            var[a, v, rng.choice(n_snp, 6, replace=False)] ^= 1
    p = rng.dirichlet(np.full(n_hla, 2.0))
    a = rng.choice(n_hla, (n_samp, 2), p=p)
    a[:n_hla, 0] = np.arange(n_hla)                    # every allele occurs
    v = rng.integers(0, 3, (n_samp, 2))
    G = var[a[:, 0], v[:, 0]] + var[a[:, 1], v[:, 1]]
    e = rng.random(G.shape) < 0.04
    G = np.where(e, (G + rng.integers(1, 3, G.shape)) % 3, G).astype(np.int32)
    G[rng.random(G.shape) < 0.03] = NA_INTEGER
    return np.ascontiguousarray(G, np.int32), a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), n_hla


def assert_same_training(got, want, what=""):
    """Two lists of trained classifiers (oracle.train's form; ``bits`` compared below each classifier's SNP count only: the
    reference leaves the bits above uninitialised)."""
    from oracle import ref as R
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        k = len(w["snpidx"])
        for key in ("snpidx", "samp_num", "hla", "freq"):
            a, b = np.ascontiguousarray(g[key]), np.ascontiguousarray(w[key])
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: classifier {i}: {key}: {a} against {b}"
        m = R.low_mask(k)
        assert np.array_equal(np.asarray(g["bits"]) & m, np.asarray(w["bits"]) & m), f"{what}: classifier {i}: haplotype bits"
        assert np.float64(g["acc"]).tobytes() == np.float64(w["acc"]).tobytes(), f"{what}: classifier {i}: accuracy"
