"""Constructed inputs for the training-side scoring kernels (hibag_amd/csrc/hibag_build.hip) at every SNP word count,
and their expected values from the oracle alone.

Random inputs do not work at these widths: the weight table is 1e-5^d and is 0 from d = 65 on, so random 128-SNP
haplotypes against random genotypes give "no best guess" and a NaN posterior for every sample -- a comparison that
passes while checking nothing.  Here every genotype is the sum of two haplotypes OF THE LIST with a few SNPs flipped or set
missing, so the true pair's cell is at distance 0...6 and the other cells are far; the properties that make a case
worth running (few degenerate samples, a top word that matters, missing codes) are asserted by
tests/test_training_inputs_host.py for every case listed below, which are the cases the GPU tests run.

Two forms:

* ``make_case``  -- one haplotype list and one genotype list: what build_set_haplo_geno takes (the plugin route);
* ``make_batch`` -- one growth step: a base genotype list with position n_snp - 1 missing, and per candidate a raw
  genotype column and a haplotype list of its own that is one bit longer than a common parent list (the batch route).

Both are deterministic in their arguments and cached: the CPU and the GPU tests of one session share the inputs and
the oracle's results, and nobody writes to them.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

NA = O.NA_INTEGER

# layout mirrors of THaplotype (32 bytes) and TGenotype (48 bytes), inst/include/LibHLA_ext.h:261-299, :311-352
THAPLO = np.dtype([("packed", "<u8", 2), ("freq", "<f8"), ("freq_f32", "<f4"), ("hla", "<i4")])
TGENO = np.dtype([("s1", "<u8", 2), ("s2", "<u8", 2), ("boot", "<i4"), ("a1", "<i4"), ("a2", "<i4"), ("pad", "<i4")])
assert THAPLO.itemsize == 32 and TGENO.itemsize == 48


def n_words(n_snp: int) -> int:
    return max(1, (n_snp + 31) // 32)


def top_word_start(n_snp: int) -> int:
    """First SNP of the last 32-bit word a classifier of n_snp SNPs uses: 32 * (nw - 1)."""
    return 32 * (n_words(n_snp) - 1)


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """[H, n_snp] 0/1 -> [H, 2] uint64, bit s of the 128-bit string = SNP s (inst/include/LibHLA_ext.h:240-255)."""
    H, k = bits.shape
    out = np.zeros((H, 2), np.uint64)
    for s in range(k):
        out[:, s >> 6] |= bits[:, s].astype(np.uint64) << np.uint64(s & 63)
    return out


def add_garbage(packed: np.ndarray, n_snp: int, rng) -> np.ndarray:
    """Random bits in every position >= n_snp of both words, like the reference's uninitialised tail
    (src/LibHLA.cpp:287-292); bit n_snp itself, the first one a wrong mask would let through, is set on every other row."""
    out = packed.copy()
    for w in range(2):
        lo = max(0, min(64, n_snp - 64 * w))              # the word's clean bits
        if lo == 64:
            continue
        mask = np.uint64(((1 << 64) - 1) ^ ((1 << lo) - 1))
        g = rng.integers(0, 1 << 63, len(out), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(out), dtype=np.uint64)
        out[:, w] |= g & mask
    if n_snp < 128:
        out[::2, n_snp >> 6] |= np.uint64(1) << np.uint64(n_snp & 63)
    return out


@dataclass(eq=False)
class HaploList:
    """A haplotype list grouped by ascending allele (CHaplotypeList, src/LibHLA.h:85-140)."""
    n_snp: int
    n_hla: int
    allele: np.ndarray                  # [H] ascending
    bits: np.ndarray                    # [H, n_snp] 0/1
    freq: np.ndarray                    # [H] positive, not normalised
    packed: np.ndarray                  # [H, 2] uint64, garbage in every bit >= n_snp

    @property
    def lens(self) -> np.ndarray:
        return np.bincount(self.allele, minlength=self.n_hla).astype(np.int32)

    def records(self) -> np.ndarray:
        r = np.zeros(len(self.allele), THAPLO)
        r["packed"] = self.packed
        r["freq"] = self.freq
        r["freq_f32"] = self.freq
        r["hla"] = self.allele
        return r


def flat_model(lists, n_snp=None) -> O.FlatModel:
    """One "classifier" per haplotype list, in the form the oracle's entry points take.  ``n_snp`` scores the lists
    truncated to their first n_snp SNPs (the packed words stay: the genotype's missing tail masks the rest)."""
    lists = list(lists)
    k = [int(l.n_snp if n_snp is None else n_snp) for l in lists]
    n_snp_c = np.array(k, np.int32)
    snp_off = np.concatenate([[0], np.cumsum(n_snp_c)]).astype(np.int32)
    hap_off = np.concatenate([[0], np.cumsum([len(l.allele) for l in lists])]).astype(np.int32)
    return O.FlatModel(
        n_hla=lists[0].n_hla, n_classifier=len(lists), n_snp_total=max(k + [1]), n_snp_c=n_snp_c, snp_off=snp_off,
        snp_index=np.concatenate([np.arange(x, dtype=np.int32) for x in k] + [np.zeros(0, np.int32)]).astype(np.int32),
        hap_off=hap_off, len_per_hla=np.stack([l.lens for l in lists]),
        bits=np.ascontiguousarray(np.concatenate([l.packed for l in lists])),
        freq=np.ascontiguousarray(np.concatenate([l.freq for l in lists])))


def encode(geno: np.ndarray, n_snp=None):
    """int genotypes [n_sample, k] -> (s1, s2) [n_sample, 2] uint64 each, with the reference's own rule (oracle.int_to_snp):
    values outside 0..2 and every position >= n_snp are missing."""
    geno = np.ascontiguousarray(geno, np.int32)
    k = geno.shape[1] if n_snp is None else n_snp
    idx = np.arange(k, dtype=np.int32)
    s1 = np.zeros((len(geno), 2), np.uint64)
    s2 = np.zeros((len(geno), 2), np.uint64)
    for s, row in enumerate(geno):
        s1[s], s2[s] = O.int_to_snp(row, idx)
    return s1, s2


# ---------------------------------------------------------------------------------------------------------------------
# construction

def _layout(n_hla, n_empty, counts):
    """Present alleles (two of them empty rows by default: the second allele and the last one) and haplotypes per
    present allele."""
    empty = [1, n_hla - 1, 3, 5][:n_empty]
    present = [h for h in range(n_hla) if h not in empty]
    assert len(present) == len(counts) and len(present) >= 2
    return present, np.repeat(present, counts).astype(np.int32)


def _list_bits(rng, width, counts, twin_from):
    """The haplotypes' bits; the LAST present allele's are copies of the one before it that differ only in positions
    >= twin_from (identical where the width has no such position)."""
    H = int(np.sum(counts))
    bits = rng.integers(0, 2, (H, width), dtype=np.uint8)
    if width > 8:
        # relatives: one founder with 1...4 SNPs changed per haplotype, anywhere in the string.  Unrelated random haplotypes
        # are ~ width / 2 apart: every cell but the true pair's is then below the last bit of the total, every posterior is
        # exactly 1, and the in-bag loss is 0 whatever the kernel adds up.
        bits[:] = bits[0]
        for h in range(H):
            bits[h, rng.choice(width, int(rng.integers(1, 5)), replace=False)] ^= 1
    if twin_from is not None:
        assert counts[-1] == counts[-2]
        n = counts[-1]
        x, y = slice(H - 2 * n, H - n), slice(H - n, H)
        bits[y] = bits[x]
        if width > twin_from:
            flip = rng.integers(0, 2, (n, width - twin_from), dtype=np.uint8)
            flip[np.arange(n), rng.integers(0, width - twin_from, n)] = 1      # at least one bit each
            bits[y, twin_from:] ^= flip
    return bits


def _freqs(rng, counts, twin):
    f = rng.uniform(0.05, 1.0, int(np.sum(counts))) * 3.0           # positive, not normalised
    if twin:
        n = counts[-1]
        f[len(f) - n:] = f[len(f) - 2 * n:len(f) - n] * 0.5          # the twin is the rarer one: without the top word it loses
    return f


def _draw_pairs(rng, pool, n_sample, x_pool=None, y_pool=None):
    """Two haplotypes of `pool` per sample; where the list has twins, the first samples carry one of them: Y, X, Y, ..."""
    i = rng.choice(pool, n_sample)
    j = rng.choice(pool, n_sample)
    if x_pool is not None:
        for s in range(min(6, n_sample)):
            i[s] = rng.choice(y_pool if s % 2 == 0 else x_pool)
    return i, j


def _flip(rng, g, width):
    """A few SNPs flipped or set missing: 0...2 per sample, whatever the width (each moves a pair's distance by at most 2)."""
    for row in g:
        for _ in range(int(rng.integers(0, 3)) if width else 0):
            p = int(rng.integers(0, width))
            row[p] = NA if rng.integers(0, 3) == 0 else (row[p] + int(rng.integers(1, 3))) % 3 if row[p] >= 0 else 0
    return g


def _bootstrap(rng, n_sample):
    if n_sample == 1:
        return np.array([1], np.int32)                                  # (one sample cannot be both: in-bag, so that every entry has work)
    boot = rng.choice(np.array([0, 0, 1, 1, 2, 3], np.int32), n_sample).astype(np.int32)
    boot[0] = 0
    boot[1] = 2
    for s, v in ((2, 0), (4, 0), (7, 0), (8, 1)):
        if s < n_sample:
            boot[s] = v
    return boot


def _far_genotype(rng, width):
    """Homozygous at every SNP: a random haplotype pair is at distance ~ width (one per SNP on average), far past the 64
    at which the weight table still holds a non-zero value."""
    return (2 * rng.integers(0, 2, width)).astype(np.int32)


@dataclass(eq=False)
class Case:
    lst: HaploList
    geno: np.ndarray                    # [n_sample, n_snp] int32: 0 / 1 / 2 / NA
    s1: np.ndarray                      # [n_sample, 2] uint64
    s2: np.ndarray
    a1: np.ndarray                      # true alleles AS STORED (either order)
    a2: np.ndarray
    boot: np.ndarray                    # [n_sample] int32, 0 = out-of-bag
    far: int = -1                       # the deliberately far sample, or -1

    def records(self) -> np.ndarray:
        return _geno_records(self.s1, self.s2, self.boot, self.a1, self.a2)


def _geno_records(s1, s2, boot, a1, a2):
    r = np.zeros(len(boot), TGENO)
    r["s1"], r["s2"], r["boot"], r["a1"], r["a2"] = s1, s2, boot, a1, a2
    return r


def _stored_order(al_i, al_j):
    a1, a2 = al_i.astype(np.int32).copy(), al_j.astype(np.int32).copy()
    odd = np.arange(len(a1)) % 2 == 1
    lo, hi = np.minimum(a1, a2), np.maximum(a1, a2)
    a1, a2 = np.where(odd, hi, lo).astype(np.int32), np.where(odd, lo, hi).astype(np.int32)    # either order must work
    return a1, a2


def _counts(rng, n_present, per_allele):
    if isinstance(per_allele, tuple) and per_allele[0] == "counts":     # explicit: ("counts", n, n, ...)
        assert len(per_allele) == n_present + 1
        return [int(v) for v in per_allele[1:]]
    if isinstance(per_allele, tuple):                                    # (lo, hi): drawn per allele
        c = [int(v) for v in rng.integers(per_allele[0], per_allele[1] + 1, n_present)]
    else:
        c = [int(per_allele)] * n_present
    c[1 if n_present > 2 else 0] = 1                                     # one allele has exactly one haplotype
    c[-1] = c[-2]                                                        # (the twins have as many as each other)
    return c


@functools.lru_cache(maxsize=None)
def make_case(n_snp, n_hla=8, per_allele=5, n_sample=65, seed=0, n_empty=2, far=False) -> Case:
    rng = np.random.default_rng([seed, n_snp, n_sample, n_hla])
    counts = _counts(rng, n_hla - n_empty, per_allele)
    present, allele = _layout(n_hla, n_empty, counts)
    twin = n_snp > 32
    bits = _list_bits(rng, n_snp, counts, top_word_start(n_snp) if twin else None)
    lst = HaploList(n_snp, n_hla, allele, bits, _freqs(rng, counts, twin), add_garbage(pack_bits(bits), n_snp, rng))
    H, nt = len(allele), counts[-1]
    i, j = _draw_pairs(rng, np.arange(H), n_sample, *((np.arange(H - 2 * nt, H - nt), np.arange(H - nt, H)) if twin else ()))
    geno = _flip(rng, bits[i].astype(np.int32) + bits[j].astype(np.int32), n_snp)
    boot = _bootstrap(rng, n_sample)
    far_s = -1
    if far:
        far_s = n_sample - 1
        geno[far_s] = _far_genotype(rng, n_snp)
        boot[far_s] = 0                   # out-of-bag: its NaN posterior then stays out of the in-bag loss
    a1, a2 = _stored_order(allele[i], allele[j])
    s1, s2 = encode(geno)
    return Case(lst, geno, s1, s2, a1, a2, boot, far_s)


@dataclass(eq=False)
class Batch:
    n_snp: int
    n_hla: int
    base: np.ndarray                    # [n_sample, n_snp] int32, last position NA
    s1: np.ndarray                      # the base genotypes' planes
    s2: np.ndarray
    a1: np.ndarray
    a2: np.ndarray
    boot: np.ndarray
    lists: list = field(default_factory=list)     # per candidate a HaploList of n_snp SNPs
    columns: np.ndarray = None          # [n_cand, n_sample] int32 raw: 0, 1, 2, NA, 3, -1
    far: int = -1

    def geno(self, c) -> np.ndarray:
        """Candidate c's genotypes: the base with SNP n_snp - 1 set from its column (TGenotype::_SetSNP,
        src/LibHLA.cpp:609-622: 0, 1, 2, anything else missing -- int_to_snp's rule for a raw value)."""
        g = self.base.copy()
        g[:, self.n_snp - 1] = self.columns[c]
        return g

    def records(self) -> np.ndarray:
        return _geno_records(self.s1, self.s2, self.boot, self.a1, self.a2)


@functools.lru_cache(maxsize=None)
def make_batch(n_snp, n_cand=3, n_hla=8, per_allele=5, n_sample=65, seed=0, n_empty=2, far=False, p_both=0.2,
               keep_of=None) -> Batch:
    """``keep_of``: per candidate how many of each allele's parent haplotypes it keeps, the first ones (default: all but a few
    dropped at random)."""
    rng = np.random.default_rng([seed, n_snp, n_sample, n_hla, n_cand])
    counts = _counts(rng, n_hla - n_empty, per_allele)
    present, p_allele = _layout(n_hla, n_empty, counts)
    twin = n_snp > 32
    Hp, w = len(p_allele), n_snp - 1
    p_bits = _list_bits(rng, w, counts, top_word_start(n_snp) if twin else None)
    p_freq = _freqs(rng, counts, twin)
    nt = counts[-1]
    is_x = np.zeros(Hp, bool)
    is_y = np.zeros(Hp, bool)
    if twin:
        is_x[Hp - 2 * nt:Hp - nt] = True
        is_y[Hp - nt:] = True
    # which parent haplotypes each candidate keeps (never none of an allele, always the twins) ...
    keeps = []
    for c in range(n_cand):
        if keep_of is not None:
            rank = np.arange(Hp) - np.searchsorted(p_allele, p_allele)       # place inside the allele's group
            keeps.append(rank < keep_of[c])
        else:
            first = np.concatenate([[True], p_allele[1:] != p_allele[:-1]])
            keeps.append(first | is_x | is_y | (rng.random(Hp) > 0.15))
    # ... and the samples: two parent haplotypes that EVERY candidate kept (a sample whose haplotype a candidate dropped is
    # far from all of that candidate's pairs at these widths: total 0), a few SNPs flipped
    common = np.logical_and.reduce(keeps)
    pools = (np.where(common & is_x)[0], np.where(common & is_y)[0]) if twin else ()
    i, j = _draw_pairs(rng, np.where(common)[0], n_sample, *pools)
    base = np.full((n_sample, n_snp), NA, np.int32)
    base[:, :w] = _flip(rng, p_bits[i].astype(np.int32) + p_bits[j].astype(np.int32), w)
    boot = _bootstrap(rng, n_sample)
    far_s = -1
    if far:
        far_s = n_sample - 1
        base[far_s, :w] = _far_genotype(rng, w)
        boot[far_s] = 0                   # out-of-bag: loss_ib stays finite
    n_of = np.bincount(p_allele, minlength=n_hla)
    lists, columns = [], np.zeros((n_cand, n_sample), np.int32)
    for c in range(n_cand):
        keep = keeps[c]
        # the bit each kept haplotype gets at the new position: 0, 1, or both (the haplotype splits in two)
        ext = rng.choice(3, Hp, p=[(1 - p_both) / 2, (1 - p_both) / 2, p_both])
        ext[(n_of[p_allele] == 1) & (ext == 2)] = 1                      # the one-haplotype allele stays one
        ext[is_x] = 0
        ext[is_y] = 1                                                    # the twins differ (also) in the candidate's bit
        rows, al, fr = [], [], []
        for h in np.where(keep)[0]:
            for b in ((0, 1) if ext[h] == 2 else (int(ext[h]),)):
                rows.append(np.concatenate([p_bits[h], [b]]).astype(np.uint8))
                al.append(p_allele[h])
                fr.append(p_freq[h] * rng.uniform(0.5, 1.5) * (0.5 if is_y[h] else 1.0))
        bits = np.array(rows, np.uint8).reshape(len(rows), n_snp)
        lists.append(HaploList(n_snp, n_hla, np.array(al, np.int32), bits, np.array(fr), add_garbage(pack_bits(bits), n_snp, rng)))
        pick = rng.integers(0, 2, (2, Hp))
        bit_of = np.where(ext == 2, pick[0], np.where(keep, ext, pick[1]))
        col = (bit_of[i] + bit_of[j]).astype(np.int32)
        for s, v in ((7, NA), (8, 3), (9, -1), (10, 0), (11, 1), (12, 2)):
            if s < n_sample and s != far_s:
                col[s] = v
        columns[c] = col
    a1, a2 = _stored_order(p_allele[i], p_allele[j])
    s1, s2 = encode(base)
    return Batch(n_snp, n_hla, base, s1, s2, a1, a2, boot, lists, columns, far_s)


# ---------------------------------------------------------------------------------------------------------------------
# expected values, from the oracle alone

@dataclass(eq=False)
class Score:
    best: np.ndarray                    # [n_sample, 2] _BestGuess (NA_INTEGER: none)
    post: np.ndarray                    # [n_sample] _PostProb of the true pair (NaN where not computed)
    total: np.ndarray                   # [n_sample] in-order total (NaN where not computed)
    acc_oob: int
    loss_ib: float


def score(lst: HaploList, geno, a1, a2, boot, n_snp=None, with_total=False) -> Score:
    """build_acc_oob = sum over the out-of-bag samples of CHLATypeList::Compare(_BestGuess, truth) (src/LibHLA.cpp:1934-1955);
    build_acc_ib = -2 * sum over the in-bag samples, in order, of count * log(_PostProb) (:1957-1979, host libm log).
    ``n_snp`` scores the first n_snp SNPs only."""
    fm = flat_model([lst], n_snp)
    s1, s2 = encode(geno, n_snp)
    n = len(boot)
    best = np.full((n, 2), NA, np.int32)
    post = np.full(n, np.nan)
    total = np.full(n, np.nan)
    acc, loglik = 0, 0.0
    for s in range(n):
        if boot[s] == 0 or with_total:
            best[s] = O.best_guess(fm, 0, s1[s], s2[s])
        if boot[s] == 0:
            acc += O.compare_hla(best[s, 0], best[s, 1], min(a1[s], a2[s]), max(a1[s], a2[s]))
        else:
            post[s] = O.post_prob(fm, 0, s1[s], s2[s], int(a1[s]), int(a2[s]))
            loglik += int(boot[s]) * (math.log(post[s]) if post[s] != 0 else -math.inf)
        if with_total:
            total[s] = O.post_prob2(fm, 0, s1[s], s2[s])[1]
    return Score(best, post, total, acc, -2 * loglik)


@functools.lru_cache(maxsize=None)
def case_score(key) -> Score:
    cs = make_case(**dict(PLUGIN_CASES[key]))
    return score(cs.lst, cs.geno, cs.a1, cs.a2, cs.boot)


@functools.lru_cache(maxsize=None)
def match_score(key) -> Score:
    cs = match_case(key)
    return score(cs.lst, cs.geno, cs.a1, cs.a2, cs.boot)


@functools.lru_cache(maxsize=None)
def haplo_matches(cs: Case) -> tuple:
    """What build_haplomatch returns, per in-bag sample in order: the (i1, i2) of _PrepHaploMatch (src/LibHLA.cpp:1569-1637),
    each index inside its allele's sub-list."""
    lst = cs.lst
    fm = flat_model([lst])
    st = np.concatenate([[0], np.cumsum(lst.lens)])
    out = []
    for s in np.where(cs.boot > 0)[0]:
        lo, hi = sorted((int(cs.a1[s]), int(cs.a2[s])))
        ref = O.prep_haplo_match(fm, 0, cs.s1[s], cs.s2[s], lo, hi)
        out.append([(int(i) - int(st[lo]), int(j) - int(st[hi])) for i, j in ref])
    return tuple(out)


def match_bound(cs: Case) -> int:
    """The library's upper bound on the number of pairs build_haplomatch can return: per in-bag sample n1 (n1 + 1) / 2 on the
    diagonal, else n1 n2.  Above 1 << 20 it sizes the pair list from a first pass's counts instead of from the bound."""
    lens = cs.lst.lens
    bound = 0
    for s in np.where(cs.boot > 0)[0]:
        lo, hi = sorted((int(cs.a1[s]), int(cs.a2[s])))
        n1, n2 = int(lens[lo]), int(lens[hi])
        bound += n1 * (n1 + 1) // 2 if lo == hi else n1 * n2
    return bound


@functools.lru_cache(maxsize=None)
def batch_scores(key) -> tuple:
    b = make_batch(**dict(BATCH_CASES[key]))
    return tuple(score(b.lists[c], b.geno(c), b.a1, b.a2, b.boot) for c in range(len(b.lists)))


def batch_expected(key, acc_floor):
    """What the batched scoring returns: every candidate's out-of-bag count, and its in-bag loss where the count reaches
    the running maximum that starts at acc_floor -- exactly 0 otherwise (src/LibHLA.cpp:2033-2034)."""
    sc = batch_scores(key)
    acc = np.array([s.acc_oob for s in sc], np.int32)
    loss = np.zeros(len(sc))
    run_max = acc_floor
    for c, s in enumerate(sc):
        if s.acc_oob < run_max:
            continue
        run_max = max(run_max, s.acc_oob)
        loss[c] = s.loss_ib
    return acc, loss


# ---------------------------------------------------------------------------------------------------------------------
# the cases the GPU tests run (tests/test_hip_training.py, tests/test_hip_train_scoring.py); every one has its
# properties checked on the CPU (tests/test_training_inputs_host.py)

def _kw(**kw):
    return tuple(sorted(kw.items()))


PLUGIN_WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
PLUGIN_SAMPLES = (1, 63, 64, 65, 130)
PLUGIN_CASES = {f"snp{k}": _kw(n_snp=k, n_sample=65, seed=11) for k in PLUGIN_WIDTHS}
PLUGIN_CASES.update({f"snp65-n{n}": _kw(n_snp=65, n_sample=n, seed=12) for n in PLUGIN_SAMPLES})
PLUGIN_CASES["far"] = _kw(n_snp=128, n_sample=65, seed=13, far=True)

BATCH_WIDTHS = (1, 32, 33, 64, 65, 96, 97, 128)
CELL_ALLELES = (2, 7, 8, 11, 63)        # present alleles p -> p (p + 1) / 2 cells: 3, 28, 36, 66, 2,016
BATCH_CASES = {f"snp{k}": _kw(n_snp=k, n_cand=3, n_sample=65, seed=21) for k in BATCH_WIDTHS}
BATCH_CASES.update({f"cells-p{p}": _kw(n_snp=40, n_cand=2, n_hla=p + 2, per_allele=(1, 2), n_sample=64, seed=22, p_both=0.0)
                    for p in CELL_ALLELES})
BATCH_CASES["cells-p20-n256"] = _kw(n_snp=40, n_cand=18, n_hla=22, per_allele=(1, 2), n_sample=256, seed=23, p_both=0.0)
# 1,100 haplotypes over 4 alleles (one of them a single haplotype) in candidate 0, the first 13 of each allele -- 40 -- in candidate 1
BATCH_CASES["direct"] = _kw(n_snp=97, n_cand=2, n_hla=6, per_allele=("counts", 367, 1, 366, 366), n_sample=64, seed=24,
                            p_both=0.0, keep_of=(1 << 20, 13))
BATCH_CASES["far"] = _kw(n_snp=128, n_cand=3, n_sample=65, seed=25, far=True)
EXEMPT = {"far"}                        # the one case (of each form) with a deliberately far sample

# build_haplomatch beyond its pair bound (1 << 20): 1,100 haplotypes over 4 alleles, so that the in-bag samples' candidate
# pairs add up to millions and the entry sizes its result from a counting pass of its own.  (A dict of its own: the
# PLUGIN_CASES lists are capped at 40 haplotypes.)
MATCH_CASES = {"two-pass": _kw(n_snp=97, n_hla=6, per_allele=("counts", 367, 1, 366, 366), n_sample=65, seed=31)}


def plugin_case(key) -> Case:
    return make_case(**dict(PLUGIN_CASES[key]))


def match_case(key) -> Case:
    return make_case(**dict(MATCH_CASES[key]))


def batch_case(key) -> Batch:
    return make_batch(**dict(BATCH_CASES[key]))
