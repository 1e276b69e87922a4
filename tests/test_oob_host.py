"""hlaOutOfBag on the host: hlaCompareAllele(full=True) on hand-built cases, and the reference's own per-classifier loop
on the oracle pinned to the out-of-bag accuracies OutOfBag.RData stores."""
import dataclasses
import math

import numpy as np
import pytest

from conftest import align_geno
from hibag_amd import NA_INTEGER, HlaAlleleClass, hlaCompareAllele
from hibag_amd.evaluate import confusion_em

LIMIT = ["A", "B", "C"]


def _hla(ids, a1, a2, prob=None):
    return HlaAlleleClass(locus="A", sample_id=list(ids), allele1=list(a1), allele2=list(a2),
                          prob=None if prob is None else np.asarray(prob, np.float64))


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)], b[~np.isnan(b)])


def test_one_miscall_and_an_allele_never_called():
    true = _hla(["s1", "s2"], ["A", "A"], ["B", "A"])
    pred = _hla(["s1", "s2"], ["A", "A"], ["C", "A"])
    r = hlaCompareAllele(true, pred, allele_limit=LIMIT, full=True)
    assert r["confusion_rows"] == ["A", "B", "C", "..."] and r["confusion_cols"] == LIMIT
    want = np.zeros((4, 3))
    want[0, 0] = 3                        # A found three times
    want[2, 1] = 1                        # true B called as C
    assert np.array_equal(r["confusion"], want)
    d = r["detail"]
    assert d["allele"] == LIMIT and "train.num" not in d
    assert np.array_equal(d["valid.num"], [3, 1, 0])
    assert np.allclose(d["valid.freq"], [0.75, 0.25, 0.0])
    assert np.array_equal(d["call.rate"], [1.0, 1.0, 0.0])
    assert _close(d["sensitivity"], [1.0, 0.0, np.nan])
    assert _close(d["specificity"], [1.0, 1.0, np.nan])
    assert _close(d["accuracy"], [1.0, 0.75, np.nan])
    assert _close(d["ppv"], [1.0, np.nan, np.nan])           # nothing was called B
    assert _close(d["npv"], [1.0, 0.75, np.nan])
    assert d["miscall"] == [None, "C", None]
    assert _close(d["miscall.prop"], [np.nan, 1.0, np.nan])
    o = r["overall"]
    assert (o["total.num.ind"], o["crt.num.ind"], o["crt.num.haplo"]) == (2, 1, 3)
    assert (o["acc.ind"], o["acc.haplo"]) == (0.5, 0.75)


def test_double_miscall_goes_through_the_em():
    # s1: both alleles missed, one call outside the limit (D -> "..."); s2: B called as C once
    true = _hla(["s1", "s2"], ["A", "A"], ["B", "B"])
    pred = _hla(["s1", "s2"], ["C", "A"], ["D", "C"])
    init = np.zeros((4, 3))
    init[0, 0] = 1
    init[2, 1] = 1
    wrong = [(0, 1, 2, 3)]
    # first the 0.5 split of each true allele over the two calls ...
    e0 = confusion_em(3, init, wrong, n_iter=0)
    assert (e0[2, 0], e0[3, 0], e0[2, 1], e0[3, 1]) == (0.5, 0.5, 1.5, 0.5)
    # ... then one EM step: true A stays split evenly, true B leans to C (1 + 1.5 / 2, 0.5 / 2)
    e1 = confusion_em(3, init, wrong, n_iter=1)
    assert (e1[2, 0], e1[3, 0], e1[2, 1], e1[3, 1]) == (0.5, 0.5, 1.75, 0.25)
    r = hlaCompareAllele(true, pred, allele_limit=LIMIT, full=True)
    want = np.zeros((4, 3))
    want[0, 0] = 1
    want[2, 0] = want[3, 0] = 0.5
    want[2, 1] = 2.0                      # 100 iterations: 2 - 2^-101 ..., rounded to two digits
    assert np.array_equal(r["confusion"], want)
    assert r["detail"]["miscall"] == ["C", "C", None]       # (A: C and "..." tie at 0.5, the first wins)
    assert _close(r["detail"]["miscall.prop"], [0.5, 1.0, np.nan])
    assert r["overall"]["crt.num.haplo"] == 1


def test_model_limit_gives_training_columns(model_oob):
    true = _hla(["s1"], ["01:01"], ["02:01"])
    r = hlaCompareAllele(true, true, allele_limit=model_oob, full=True)
    d = r["detail"]
    assert d["allele"] == list(model_oob.hla_allele)
    assert np.allclose(d["train.num"], 2 * np.asarray(model_oob.hla_freq) * model_oob.n_samp)


@pytest.mark.parametrize("thr", [float("nan"), 0.5])
def test_full_false_is_the_overall_of_full_true(thr):
    true = _hla(["s1", "s2", "s3"], ["A", "A", "B"], ["B", "A", "C"])
    pred = _hla(["s1", "s2", "s3"], ["A", "C", "B"], ["B", "D", "C"], prob=[0.9, 0.4, 0.6])
    short = hlaCompareAllele(true, pred, allele_limit=LIMIT, call_threshold=thr)
    full = hlaCompareAllele(true, pred, allele_limit=LIMIT, call_threshold=thr, full=True)
    assert set(full) >= {"overall", "confusion", "detail"}
    assert full["overall"].keys() == short.keys()
    assert all(short[k] == full["overall"][k] or (math.isnan(short[k]) and math.isnan(full["overall"][k])) for k in short)


# ---- the reference's loop (R/HIBAG.R:1320-1334) on the oracle ---------------------------------------------------------

def oracle_oob(oracle, model, G, avx2=False, n_threads=1):
    """Classifier by classifier: a one-classifier model predicts its OOB samples (vote "prob").  [C, n] arrays.
    `avx2` / `n_threads`: the oracle's AVX2 port (pinned equal to the scalar restatement), for cohorts at size."""
    C, n = len(model.classifiers), G.shape[0]
    h1 = np.full((C, n), NA_INTEGER, np.int32)
    h2 = np.full((C, n), NA_INTEGER, np.int32)
    prob = np.zeros((C, n))
    for c, cls in enumerate(model.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        fm = oracle.flatten(dataclasses.replace(model, classifiers=[cls]))
        r = oracle.predict(fm, G[oob], 1, want_dosage=False, want_prob=False, avx2=avx2, n_threads=n_threads)
        h1[c, oob], h2[c, oob], prob[c, oob] = r["h1"], r["h2"], r["prob"]
    return {"h1": h1, "h2": h2, "prob": prob}


def test_oracle_loop_reproduces_the_stored_oob_accuracy(oracle, model_oob, hapmap_geno, hla_type_table):
    G = align_geno(model_oob, hapmap_geno)
    got = oracle_oob(oracle, model_oob, G)
    tab = {s: (a, b) for s, a, b in zip(hla_type_table["sample.id"], hla_type_table["A.1"], hla_type_table["A.2"])}
    idx = {a: i for i, a in enumerate(model_oob.hla_allele)}
    full_call, exact = [], []
    for c, cls in enumerate(model_oob.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        if not np.all(got["h1"][c, oob] != NA_INTEGER):
            continue
        full_call.append(c)
        correct = 0
        for k in oob:
            t1, t2 = tab[model_oob.sample_id[k]]
            correct += oracle.compare_hla(got["h1"][c, k], got["h2"][c, k], idx.get(t1, -2), idx.get(t2, -3))
        if 0.5 * correct / len(oob) == cls.outofbag_acc:
            exact.append(c)
    assert full_call == [c for c in range(100) if c != 98]
    assert exact == full_call
    # classifier 98: two of its OOB samples miss every one of its SNPs -- hlaPredict calls nothing there
    oob98 = np.flatnonzero(np.asarray(model_oob.classifiers[98].samp_num) == 0)
    assert int(np.sum(got["h1"][98, oob98] == NA_INTEGER)) == 2


# ---- T-ties: cells that the one-classifier transform merges -----------------------------------------------------------
# A one-classifier model's call is the first strict maximum of T(p) = (0 + p * w) * (1 / w), p = cell * (1 / total),
# w = typed SNPs / SNPs (src/LibHLA.cpp:1497-1518, 1549-1566, 2418-2431).  T can map cells an ulp apart to one value,
# and then the EARLIER cell wins.  With one haplotype "00...0" per allele every pair is at distance 0, so the cells are
# products of frequencies alone, and near-equal frequencies put the largest cells (0, j) a few ulps apart.

TIE_SNPS = 120
TIE_VARIANTS = ("basic", "ring", "first")
TIE_RING_START = 11          # "ring": cells 0 .. 10 are eleven rising records before the near-equal ones
_EPS = 2.0 ** -52


def _tie_freqs(rng, variant):
    """basic: f0 and seven near-equal f_j (records: (0,0), (0,1) and the (0,j) that still rise).
    ring: ten clearly rising f_j first -- eleven records precede the near-equal cells, so the earliest tied record has
    left slot 1 (the first record) and sits in the ring of the six latest.
    first: f_j near f0 / 2, so 2 f0 f_j lies an ulp or two from f0^2: the first record, cell (0,0), ties with the maximum."""
    if variant == "basic":
        return np.concatenate([[0.15], 0.11 * (1 + rng.integers(0, 6, 7) * _EPS)])
    if variant == "ring":
        return np.concatenate([[0.15], 0.05 + 0.004 * np.arange(1, TIE_RING_START), 0.11 * (1 + rng.integers(0, 6, 7) * _EPS)])
    f0 = rng.uniform(0.1, 0.3)
    return np.concatenate([[f0], f0 / 2 * (1 + rng.integers(0, 2, 7) * _EPS)])


def tie_case(snp_counts, seed, per=6):
    """A model of `per` classifiers per (variant, SNP count) -- classifier i has variant TIE_VARIANTS[i // per %
    3] -- 256 samples typed 0 at growing prefixes and at random subsets of the SNPs (NA elsewhere: weights typed / k),
    and bootstrap counts that leave four samples in five out of bag.  Returns (model, G, samp_num, variant per classifier)."""
    from hibag_amd.model import Classifier, HlaAttrBagObj
    rng = np.random.default_rng(seed)
    cls, kind = [], []
    for k in snp_counts:
        for v in TIE_VARIANTS:
            for _ in range(per):
                f = _tie_freqs(rng, v)
                cls.append(Classifier(snpidx=np.sort(rng.choice(TIE_SNPS, k, replace=False)), freq=f,
                                      hla=np.arange(len(f)), haplo=["0" * k] * len(f)))
                kind.append(v)
    n_hla = max(len(c.freq) for c in cls)
    n = 256
    G = np.full((n, TIE_SNPS), NA_INTEGER, np.int32)
    for t in range(1, TIE_SNPS + 1):
        G[t - 1, :t] = 0
    for s in range(TIE_SNPS, n):
        G[s, rng.random(TIE_SNPS) < rng.uniform(0.05, 0.95)] = 0
    samp_num = np.zeros((len(cls), n), np.int32)
    for c in range(len(cls)):
        samp_num[c, (np.arange(n) + c) % 5 == 0] = 1
        cls[c].samp_num = samp_num[c]
    model = HlaAttrBagObj(n_samp=n, n_snp=TIE_SNPS, hla_allele=[f"{a:02d}" for a in range(n_hla)], classifiers=cls,
                          sample_id=[f"s{i}" for i in range(n)])
    return model, G, samp_num, kind


def _cell(h1, h2, n_hla):
    return h1 * n_hla - h1 * (h1 - 1) // 2 + (h2 - h1)


def tie_calls(oracle, model, G, want):
    """[C, n] bool: the oracle's out-of-bag call (`want`, from oracle_oob) is NOT the first maximum of the raw cells
    p (oracle.post_prob2) -- a T-tie decided it -- and [C, n] int: the cell it called (-1: none).  Checks on the way that
    the call is the first strict maximum of T restated here, and that `prob` is its value."""
    C, n = want["h1"].shape
    tie = np.zeros((C, n), bool)
    called = np.full((C, n), -1)
    for c, cls in enumerate(model.classifiers):
        fm = oracle.flatten(dataclasses.replace(model, classifiers=[cls]))
        idx = np.asarray(cls.snpidx)
        for s in np.flatnonzero(want["h1"][c] != NA_INTEGER):
            cells, _ = oracle.post_prob2(fm, 0, *oracle.int_to_snp(G[s], idx))       # (p = cell * (1 / total))
            w = np.count_nonzero((G[s, idx] >= 0) & (G[s, idx] <= 2)) / len(idx)
            T = (0.0 + cells * w) * (1 / w)
            p = _cell(int(want["h1"][c, s]), int(want["h2"][c, s]), model.n_hla)
            assert p == int(np.argmax(T)) and T[p] == want["prob"][c, s], (c, s)
            called[c, s] = p
            tie[c, s] = p != int(np.argmax(cells))
    return tie, called


@pytest.mark.parametrize("snp_counts,seed", [((10, 20, 27), 1), ((40, 84), 2), ((113, 120), 3)])
def test_t_ties_are_reached_on_the_oracle(oracle, snp_counts, seed):
    """The crafted cases of tests/test_hip_oob.py::test_t_ties really are T-ties in each variant: calls that are not
    the raw first maximum, in the ring after more than seven records, and at the first record."""
    model, G, samp_num, kind = tie_case(snp_counts, seed)
    want = oracle_oob(oracle, model, G)
    tie, called = tie_calls(oracle, model, G, want)
    kind = np.array(kind)
    for v in TIE_VARIANTS:
        assert tie[kind == v].sum() >= 5, (v, int(tie[kind == v].sum()))
    ring = tie[kind == "ring"] & (called[kind == "ring"] >= TIE_RING_START)
    assert ring.sum() >= 5
    first = tie[kind == "first"] & (called[kind == "first"] == 0)
    assert first.sum() >= 5
    assert np.array_equal(oracle_oob(oracle, model, G, avx2=True, n_threads=8)["prob"], want["prob"])
