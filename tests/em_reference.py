"""A plain reference of the EM haplotype-frequency fit of one candidate SNP, and the constructed growth steps the device
kernel (k_em_fit, hibag_amd/csrc/hibag_em.hip) is compared with it on.

``fit`` is CAlg_EM::PrepareNewSNP + ExpectationMaximization (src/LibHLA.cpp:1127-1255) in Python floats, in the reference's
order and with its operations as oracle/hibag_oracle_train.c restates them (expectation_maximization with prepare_new_snp's
flags and double_haplos_init_freq); tests/test_em_host.py holds it to the oracle's own trainer bit for bit
(oracle_em_fit).  Nothing here is vectorised: every sum is a Python loop in the reference's order.

The kernel decides the stopping test with a margin for its own log() and hands a candidate back (status 2) where the test
comes closer to its tolerance than the kernel's documented slack.  ``fit`` therefore also returns, per iteration, how far
the test was from the tolerance in units of that slack; a fit is DECIDED when every iteration keeps more than 4 x the
slack.  The kernel's derivation leaves a factor 4 between the true error of its log-likelihood and the slack, so a decided
fit must come back with status 1 -- the cap on hand-backs among decided candidates is zero -- and an undecided one is
not compared (the table below has none except the two deliberate hand-back cases; tests/test_em_host.py asserts that).

The cases are built from fixed seeds and cached: the CPU and the GPU tests of one session share the inputs and the
reference's results, and nobody writes to them.
"""

from __future__ import annotations

import functools
import math
import sys
from dataclasses import dataclass

import numpy as np

EM_MAX_ITER = 500                    # src/LibHLA.cpp:98
EM_INIT_VAL_FRAC = 0.001             # :100
EM_FUNC_RELTOL = math.sqrt(sys.float_info.epsilon)      # :102
DECIDED_FACTOR = 4.0
_U = 2.0 ** -53

# the list lengths that reach every loop edge of phase C (padding to 4, the 16- and 4-wide staged loops, the 8-entry
# pipelined gather and both of its exits), and the pairs-per-sample counts around psum's 16-wide groups
LIST_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33)
PAIRS_PER_SAMPLE = (1, 3, 4, 15, 16, 17, 31, 32, 33, 48)
SAMPLE_COUNTS = (1, 2, 7, 8, 9, 16, 17, 33, 64, 65, 100, 257)
STAGED, GATHER = 1, 2


def _log(x: float) -> float:
    """C's log(): -inf at 0 and NaN below it or at NaN, no exception."""
    if x > 0:
        return math.log(x)
    return -math.inf if x == 0 else math.nan


def fit(h1, h2, off, boot, geno_c, cur_freq, afreq, n_samp_total, two_last=False):
    """One candidate's fit.  h1 / h2 [n_pair] index the doubled haplotype list (2 i: allele 0 of the new SNP, 2 i + 1:
    allele 1), sample i owns pairs off[i]:off[i + 1], has count boot[i] and genotype geno_c[i] (0, 1, 2; else missing).
    Returns (freq [n_hap] float64, iters, diag): iters is the loop counter at the stop (the 0-based number of the iteration
    whose frequencies are returned, 501 where 500 iterations did not converge), diag the per-iteration record
    ``loglik``, ``T`` (sum of |term|), ``margin`` (| |dL| - tol | over the device's slack; inf for iteration 0) and the
    summary ``decided``.
    two_last=True is NOT the reference: it doubles a heterozygous pair's product AFTER multiplying, 2 * (f1 * f2), which
    gives other bits only where f1 * f2 is subnormal.  tests/test_em_host.py uses it to show that the underflow cases
    below can tell the two apart."""
    h1 = [int(v) for v in h1]
    h2 = [int(v) for v in h2]
    off = [int(v) for v in off]
    n_ib, n_hap = len(boot), 2 * len(cur_freq)
    # double_haplos_init_freq
    p1 = float(afreq)
    p0 = 1 - p1
    f = [0.0] * n_hap
    for i, cf in enumerate(cur_freq):
        f[2 * i] = p0 * float(cf) + EM_INIT_VAL_FRAC
        f[2 * i + 1] = p1 * float(cf) + EM_INIT_VAL_FRAC
    # prepare_new_snp's flags: the pairs that take part, per sample, in pair order
    samples = []
    for i in range(n_ib):
        g = int(geno_c[i])
        typed = 0 <= g <= 2
        prs = [(h1[j], h2[j]) for j in range(off[i], off[i + 1]) if not typed or (h1[j] & 1) + (h2[j] & 1) == g]
        samples.append((int(boot[i]), prs))
    scale = 0.5 / int(n_samp_total)
    loglik, conv_tol = -1e+30, 0.0
    logliks, Ts = [], []
    iters = EM_MAX_ITER + 1
    for it in range(EM_MAX_ITER + 1):
        old_loglik = loglik
        old, new = f, [0.0] * n_hap
        terms, scaled = [], []
        for b, prs in samples:
            psum = 0.0
            gf = []
            for a, c in prs:
                if a == c:
                    x = old[a] * old[c]
                else:
                    x = (2 * old[a] * old[c]) if not two_last else (2 * (old[a] * old[c]))
                gf.append(x)
                psum += x
            terms.append(b * _log(psum))
            r = b / psum if psum != 0 else math.inf
            scaled.append([x * r for x in gf])
        loglik = 0.0
        for term, (b, prs), gf in zip(terms, samples, scaled):
            loglik += term
            for (a, c), x in zip(prs, gf):
                new[a] += x
                new[c] += x
        f = [x * scale for x in new]
        logliks.append(loglik)
        Ts.append(sum(abs(t) for t in terms))
        if it > 0:
            if abs(loglik - old_loglik) <= conv_tol:
                iters = it
                break
        else:
            conv_tol = EM_FUNC_RELTOL * (abs(loglik) + EM_FUNC_RELTOL)
            if conv_tol < 0:
                conv_tol = 0.0
    # the device's slack (header of hibag_em.hip): bound_k + bound_(k-1) + sqrt(eps) bound_0, bound = 8 u (n_ib + 4) T
    bound = [8.0 * _U * (n_ib + 4) * t for t in Ts]
    margin = [math.inf]
    for k in range(1, len(logliks)):
        slack = bound[k] + bound[k - 1] + EM_FUNC_RELTOL * bound[0]
        d = abs(abs(logliks[k] - logliks[k - 1]) - conv_tol)
        margin.append(d / slack if slack > 0 and math.isfinite(d) else 0.0)
    decided = math.isfinite(logliks[0]) and all(m > DECIDED_FACTOR for m in margin)
    diag = dict(loglik=logliks, T=Ts, margin=margin, decided=decided, conv_tol=conv_tol)
    return np.array(f, np.float64), iters, diag


# ---- the kernel's LDS budget, restated from the header of hibag_em.hip ---------------------------------------------

EM_LDS_BYTES = 156 * 1024


def lds_bytes(n_ib: int, n_pair: int, n_hap: int, staged: bool) -> int:
    """Bytes of LDS a step needs: two frequency vectors, G with its +0.0 slot, two term buffers, boot / psum, the packed
    pairs, the offsets, the counts, the lists' offsets, the lists (gather: 4-byte offsets of up to 2 n_pair + 4 n_hap
    entries with padding; staged: two 16-bit positions per pair), each pair's sample, and (staged) the lists' own values.
    Every array starts on a multiple of 8."""
    up = lambda v: (v + 7) & ~7
    n_ent = 2 * n_pair + 4 * n_hap
    parts = [n_hap * 8, n_hap * 8, (n_pair + 1) * 8 + 8, n_ib * 16, n_ib * 8, n_pair * 4, (n_ib + 1) * 4, n_ib * 4, (n_hap + 1) * 4,
             (4 * n_pair + 16) if staged else (n_ent * 4 + 16), n_pair * 2, (n_ent * 8 + 16) if staged else 0]
    return sum(up(p) for p in parts)


def expected_layout(n_ib: int, n_pair: int, n_hap: int) -> int:
    """0 = the host's, 1 = staged, 2 = gather."""
    if not (0 < n_ib <= 65535 and n_pair <= 65535 and n_hap <= 16384 and lds_bytes(n_ib, n_pair, n_hap, False) + 64 <= EM_LDS_BYTES):
        return 0
    if 2 * n_pair + 4 * n_hap <= 65535 and lds_bytes(n_ib, n_pair, n_hap, True) + 64 <= EM_LDS_BYTES:
        return STAGED
    return GATHER


# ---- the case table --------------------------------------------------------------------------------------------------

@dataclass(eq=False)
class Case:
    name: str
    n_ib: int
    n_pair: int
    n_hap: int
    n_samp_total: int
    h1: np.ndarray              # [n_pair] int32
    h2: np.ndarray
    off: np.ndarray             # [n_ib + 1] int32
    boot: np.ndarray            # [n_ib] int32, 1..9
    cur_freq: np.ndarray        # [n_hap / 2]
    geno: np.ndarray            # [n_cand][n_ib] int8: 0, 1, 2, 3 = missing
    afreq: np.ndarray           # [n_cand]
    layout: int                 # what the step's dimensions select
    hand_back: bool = False     # the first log-likelihood is -inf for every candidate: the kernel's answer is status 2

    @property
    def n_cand(self) -> int:
        return len(self.afreq)

    def pairs_per_sample(self):
        return np.diff(self.off)

    def list_lengths(self):
        """Entries of every doubled haplotype's transposed list, a homozygous pair counted twice."""
        return np.bincount(self.h1, minlength=self.n_hap) + np.bincount(self.h2, minlength=self.n_hap)


def _expand(a: int, b: int):
    """The doubled pairs of base pair (a, b) of the current list, in the order PrepareHaplotypes yields them (first
    haplotype outer, second inner; within one allele's range only h2 >= h1)."""
    if a == b:
        return [(2 * a, 2 * a), (2 * a, 2 * a + 1), (2 * a + 1, 2 * a + 1)]
    return [(2 * a + x, 2 * b + y) for x in (0, 1) for y in (0, 1)]


def _sample_pairs(rng, n_cur: int, n_base: int = 0, k: int = 0):
    """A sample's doubled pairs: n_base distinct base pairs expanded, or exactly k pairs -- an arbitrary subset, in order,
    of as many expanded base pairs as it takes."""
    seen, out = set(), []
    while (len(seen) < n_base) if n_base else (len(out) < k):
        a, b = sorted(int(v) for v in rng.integers(0, n_cur, 2))
        if (a, b) in seen:
            if len(seen) == n_cur * (n_cur + 1) // 2:
                raise ValueError("more base pairs asked for than the list has")
            continue
        seen.add((a, b))
        out += _expand(a, b)
    if k and len(out) > k:
        keep = np.sort(rng.choice(len(out), k, replace=False))
        out = [out[i] for i in keep]
    return out


def afreq_in_bag(geno_c, boot) -> float:
    """prepare_new_snp: the candidate's allele frequency over the typed in-bag samples, weighted by their counts."""
    allele_cnt = valid_cnt = 0
    for g, dup in zip(geno_c, boot):
        if 0 <= g <= 2:
            allele_cnt += int(g) * int(dup)
            valid_cnt += 2 * int(dup)
    return allele_cnt / valid_cnt if valid_cnt else math.nan


def _candidates(rng, per_sample, boot, n_typed: int, all_missing: bool = True, missing: float = 0.05):
    """n_typed candidates of genotypes 0 / 1 / 2 with about 5 % missing, each sample's genotype one that at least one of
    its pairs is compatible with (no sample's psum is 0), none monomorphic in the bag; then the all-missing candidate.
    That one never reaches a fit in training (its allele count is 0, so the driver skips it like the reference,
    src/LibHLA.cpp:1140-1143) and 0 / 0 is no frequency: it gets afreq = 0.5.  It is here because it is the one
    candidate for which EVERY pair of the set takes part."""
    n_ib = len(per_sample)
    sums = [sorted({(a & 1) + (b & 1) for a, b in prs}) for prs in per_sample]
    geno, afreq = [], []
    while len(geno) < n_typed:
        p = rng.uniform(0.15, 0.85)
        g = np.empty(n_ib, np.int8)
        for i in range(n_ib):
            want = int(rng.random() < p) + int(rng.random() < p)
            g[i] = want if want in sums[i] else sums[i][int(rng.integers(0, len(sums[i])))]
            if rng.random() < missing:
                g[i] = 3
        af = afreq_in_bag(g, boot)
        if not (0 < af < 1):
            continue
        geno.append(g)
        afreq.append(af)
    if all_missing:
        geno.append(np.full(n_ib, 3, np.int8))
        afreq.append(0.5)
    return np.ascontiguousarray(np.stack(geno)), np.array(afreq, np.float64)


def _assemble(name, rng, per_sample, n_cur, n_typed, hand_back=False, all_missing=True, force_geno=None):
    n_ib = len(per_sample)
    off = np.concatenate([[0], np.cumsum([len(p) for p in per_sample])]).astype(np.int32)
    flat = [pr for prs in per_sample for pr in prs]
    h1 = np.array([p[0] for p in flat], np.int32)
    h2 = np.array([p[1] for p in flat], np.int32)
    boot = rng.integers(1, 10, n_ib).astype(np.int32)
    n_samp_total = n_ib + 1 + n_ib // 3
    cur = rng.random(n_cur) + 0.05
    cur = cur / cur.sum()
    typed_from = [prs if prs else [(0, 0), (0, 1), (1, 1)] for prs in per_sample]       # (a sample without pairs: any genotype)
    geno, afreq = _candidates(rng, typed_from, boot, n_typed, all_missing)
    if force_geno is not None:
        for i, g in force_geno.items():
            geno[:, i] = g
        afreq = np.array([afreq_in_bag(g, boot) for g in geno], np.float64)
        assert np.all((afreq > 0) & (afreq < 1))
    n_pair, n_hap = len(flat), 2 * n_cur
    return Case(name, n_ib, n_pair, n_hap, n_samp_total, h1, h2, off, boot, cur, geno, afreq,
                expected_layout(n_ib, n_pair, n_hap), hand_back)


def _from_degrees(rng, degree, loops):
    """Pairs (h1 <= h2) in which haplotype h occurs degree[h] times, a homozygous pair (h, h) counting twice; loops[h] of
    them are asked for first, the rest joins the two haplotypes with the most occurrences left (a last haplotype left
    alone takes homozygous pairs).  The order is shuffled."""
    left = list(degree)
    assert sum(left) % 2 == 0
    pairs = []
    for h, n in loops.items():
        assert left[h] >= 2 * n
        pairs += [(h, h)] * n
        left[h] -= 2 * n
    while True:
        order = sorted(range(len(left)), key=lambda h: -left[h])
        a, b = order[0], order[1]
        if left[a] == 0:
            break
        if left[b] == 0:
            assert left[a] % 2 == 0
            pairs += [(a, a)] * (left[a] // 2)
            left[a] = 0
            break
        pairs.append((min(a, b), max(a, b)))
        left[a] -= 1
        left[b] -= 1
    return [pairs[i] for i in rng.permutation(len(pairs))]


def _deal(rng, pairs, n_ib):
    """The pairs dealt to n_ib samples in order, every sample at least one."""
    cuts = np.sort(rng.choice(np.arange(1, len(pairs)), n_ib - 1, replace=False))
    return [pairs[lo:hi] for lo, hi in zip([0, *cuts], [*cuts, len(pairs)])]


def _list_case(name, seed, n_cur, n_ib, n_pair=None):
    """Haplotypes whose lists have every length of LIST_LENGTHS (two haplotypes each, several with homozygous pairs); with
    n_pair given, the other haplotypes share what is left of 2 n_pair occurrences."""
    rng = np.random.default_rng(seed)
    n_hap = 2 * n_cur
    degree = [d for d in LIST_LENGTHS for _ in (0, 1)]
    assert len(degree) <= n_hap
    loops = {2 * k + 1: d // 2 if d in (2, 3) else min(d // 2, 1 + k % 3) for k, d in enumerate(LIST_LENGTHS) if d >= 2}
    if n_pair is None:
        degree += [0] * (n_hap - len(degree))
    else:
        rest, n_big = 2 * n_pair - sum(degree), n_hap - len(degree)
        degree += [rest // n_big + (1 if k < rest % n_big else 0) for k in range(n_big)]
    order = rng.permutation(n_hap)                       # which haplotype gets which length
    pairs = [tuple(sorted((int(order[a]), int(order[b])))) for a, b in _from_degrees(rng, degree, loops)]
    c = _assemble(name, rng, _deal(rng, pairs, n_ib), n_cur, 2)
    assert sorted(c.list_lengths()) == sorted(degree)
    return c


# The fast and the slow fits: name -> (seed, n_ib, n_cur, base pairs per sample, missing share of the typed candidate).  Found
# by running the oracle's fit over seeds 9000.. of exactly this constructor (400 seeds, seconds of CPU time) and keeping one
# per kind and parity of the iteration count of candidate 0: 16 and 13, 386 and 239, and one that never meets the stopping
# test (501: all 500 iterations, the kernel's `res = nxt` exit).  tests/test_em_host.py pins the counts.
SPEED_CASES = {
    "fast_even": (9156, 23, 3, 1, 0.05),
    "fast_odd": (9131, 45, 4, 1, 0.0),
    "slow_even": (9013, 22, 6, 3, 0.9),
    "slow_odd": (9002, 36, 7, 4, 0.05),
    "capped": (9006, 26, 4, 2, 0.05),
}
SPEED_ITERS = {"fast_even": 16, "fast_odd": 13, "slow_even": 386, "slow_odd": 239, "capped": 501}


# Fits that end with a haplotype's frequency in the subnormal range (same constructor, seeds 20000..; found by comparing the
# oracle's fit with a copy that doubles after the product): the only inputs on which 2 * f1 * f2 evaluated left to right
# and 2 * (f1 * f2) differ, since doubling is exact until the product underflows -- and the device's FP64 subnormals at work.
UNDERFLOW_CASES = {
    "underflow_a": (20761, 6, 3, 3, 0.0),
    "underflow_b": (29495, 9, 5, 2, 0.0),
    "underflow_c": (33052, 13, 7, 1, 0.6),
}


def _build_cases():
    cases = {}

    def add(c):
        assert c.name not in cases
        cases[c.name] = c

    # sample counts: ~3 base pairs each, 3 typed candidates + the all-missing one
    for n_ib in SAMPLE_COUNTS:
        rng = np.random.default_rng(1000 + n_ib)
        per = [_sample_pairs(rng, 6, n_base=int(rng.integers(2, 5))) for _ in range(n_ib)]
        add(_assemble(f"n{n_ib}", rng, per, 6, 3))
    # pairs per sample: every count twice
    rng = np.random.default_rng(2000)
    per = [_sample_pairs(rng, 10, k=k) for k in PAIRS_PER_SAMPLE + PAIRS_PER_SAMPLE[::-1]]
    add(_assemble("psum", rng, per, 10, 3))
    # list lengths, in both layouts
    add(_list_case("lists_staged", 3000, 17, 50))
    add(_list_case("lists_gather", 3001, 30, 300, n_pair=5001))
    # many pairs
    for n_pair, n_ib, n_cur, seed in ((4101, 200, 20, 4000), (1003, 60, 10, 4001)):
        rng = np.random.default_rng(seed)
        k = rng.multinomial(n_pair - 8 * n_ib, np.ones(n_ib) / n_ib) + 8
        add(_assemble(f"pairs{n_pair}", rng, [_sample_pairs(rng, n_cur, k=int(v)) for v in k], n_cur, 2))
    # many samples
    rng = np.random.default_rng(5000)
    add(_assemble("samples1000", rng, [_sample_pairs(rng, 12, k=int(rng.integers(2, 5))) for _ in range(1000)], 12, 2))
    # many haplotypes: most lists empty, indices past 2,048, the last haplotype in use
    rng = np.random.default_rng(6000)
    per = [_sample_pairs(rng, 2000, k=3) for _ in range(100)]
    per[-1] = [(3998, 3999), (3999, 3999), (2048, 3999)]
    add(_assemble("haps4000", rng, per, 2000, 2))
    # candidates: 1, 8, 40 on one set
    rng = np.random.default_rng(7000)
    base = _assemble("cand40", rng, [_sample_pairs(rng, 5, n_base=3) for _ in range(33)], 5, 39)
    for n in (1, 8, 40):
        sel = list(range(n - 1)) + [39]
        add(Case(f"cand{n}", base.n_ib, base.n_pair, base.n_hap, base.n_samp_total, base.h1, base.h2, base.off, base.boot,
                 base.cur_freq, np.ascontiguousarray(base.geno[sel]), base.afreq[sel].copy(), base.layout))
    # fast and slow
    for name, (seed, n_ib, n_cur, n_base, miss) in SPEED_CASES.items():
        add(speed_case(name, seed, n_ib, n_cur, n_base, miss))
    for name, args in UNDERFLOW_CASES.items():
        add(speed_case(name, *args))
    # hand-back: a sample with no pair at all; a sample none of whose pairs is compatible with its genotype
    rng = np.random.default_rng(8000)
    per = [_sample_pairs(rng, 6, n_base=3) for _ in range(9)]
    per[4] = []
    add(_assemble("hb_empty", rng, per, 6, 2, hand_back=True))
    rng = np.random.default_rng(8001)
    per = [_sample_pairs(rng, 6, n_base=3) for _ in range(9)]
    per[6] = [(2, 4), (2, 6), (8, 10)]                  # allele 0 on both haplotypes of every pair, genotype 2 at every candidate
    add(_assemble("hb_incompatible", rng, per, 6, 3, hand_back=True, all_missing=False, force_geno={6: 2}))
    return cases


def speed_case(name, seed, n_ib, n_cur, n_base, miss):
    """A small step with one typed candidate and the all-missing one; `miss` = the typed candidate's share of missing
    genotypes (what makes a fit slow: little to tell the two new alleles apart by)."""
    rng = np.random.default_rng(seed)
    per = [_sample_pairs(rng, n_cur, n_base=n_base) for _ in range(n_ib)]
    n_ib = len(per)
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    flat = [pr for prs in per for pr in prs]
    boot = rng.integers(1, 10, n_ib).astype(np.int32)
    cur = rng.random(n_cur) + 0.05
    cur = cur / cur.sum()
    geno, afreq = _candidates(rng, per, boot, 1, True, miss)
    return Case(name, n_ib, len(flat), 2 * n_cur, n_ib + 1 + n_ib // 3, np.array([p[0] for p in flat], np.int32),
                np.array([p[1] for p in flat], np.int32), off, boot, cur, geno, afreq, expected_layout(n_ib, len(flat), 2 * n_cur))




@functools.lru_cache(maxsize=None)
def case_table():
    return _build_cases()


def case(name: str) -> Case:
    return case_table()[name]


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """[(freq, iters, diag)] per candidate of the case, computed once."""
    c = case(name)
    return [fit(c.h1, c.h2, c.off, c.boot, c.geno[k], c.cur_freq, float(c.afreq[k]), c.n_samp_total) for k in range(c.n_cand)]
