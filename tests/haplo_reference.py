"""hlaHaplotypes restated in plain Python and numpy, independent of hibag_amd/haplo.py and of the
device code: candidates and trimming, state enumeration by nested loops, the dictionary, the summation rule S64 with its
order written out, the EM, the calls.  numpy is used only where the order of operations is not in question: element-wise
products and quotients of float64 are the same IEEE operations one element at a time."""
import itertools
import math

import numpy as np

NA = -2147483648


def s64(x):
    """S64: 64 partial sums striding the list, each added in order, then p_j += p_{j + h} for h = 32 .. 1."""
    x = [float(v) for v in x]
    p = [0.0] * 64
    for j in range(min(64, len(x))):
        acc = x[j]
        for i in range(j + 64, len(x), 64):
            acc = acc + x[i]
        p[j] = acc
    h = 32
    while h >= 1:
        for j in range(h):
            p[j] = p[j] + p[j + h]
        h //= 2
    return p[0]


def _s64_rows(x):
    """s64 of one list, the strided part on whole rows of 64 (the same additions in the same order)."""
    x = np.asarray(x, np.float64)
    p = np.zeros(64)
    for i in range(0, len(x), 64):
        c = x[i:i + 64]
        p[:len(c)] = c if i == 0 else p[:len(c)] + c
    for h in (32, 16, 8, 4, 2, 1):
        p[:h] = p[:h] + p[h:2 * h]
    return float(p[0])


def candidates(h1, h2, prob):
    """Per sample and locus the list of (lo, hi, p) in rank order from arrays [L][n][k]: NA ranks and probability 0 skipped."""
    L, n, k = np.shape(h1)
    out = []
    for s in range(n):
        row = []
        for l in range(L):
            c = []
            for r in range(k):
                a, b, p = int(h1[l][s][r]), int(h2[l][s][r]), float(prob[l][s][r])
                if a == NA or b == NA or not p > 0.0:
                    continue
                c.append((min(a, b), max(a, b), p))
            row.append(c)
        out.append(row)
    return out


def closed_count(cands):
    """(prod (hom + 2 het) + prod hom) / 2 for one sample's candidate lists."""
    a = b = 1
    for c in cands:
        hom = sum(1 for x in c if x[0] == x[1])
        het = len(c) - hom
        a *= hom + 2 * het
        b *= hom
    return (a + b) // 2


def trim(cands, min_prob, max_states):
    """One sample's lists trimmed; returns (lists, dropped (locus, rank) in the order they went).  ValueError if rank 0
    alone exceeds the cap."""
    live = [[(r, x) for r, x in enumerate(c) if r == 0 or x[2] >= min_prob] for c in cands]
    gone = [(l, r) for l, c in enumerate(cands) for r, x in enumerate(c) if r >= 1 and x[2] < min_prob]
    while closed_count([[x for _, x in c] for c in live]) > max_states:
        best = None
        for l, c in enumerate(live):
            for r, x in c:
                if r == 0:
                    continue
                # the smallest p; of equals the highest locus, then the highest rank
                if best is None or x[2] < best[0] or (x[2] == best[0] and (l > best[1] or (l == best[1] and r > best[2]))):
                    best = (x[2], l, r)
        if best is None:
            raise ValueError("rank 0 alone exceeds max_states")
        live[best[1]] = [(r, x) for r, x in live[best[1]] if r != best[2]]
        gone.append((best[1], best[2]))
    return [[x for _, x in c] for c in live], gone


def enumerate_states(cands):
    """One sample's states in order: (w c, key A, key B, alleles A, alleles B)."""
    L = len(cands)
    out = []
    for combo in itertools.product(*cands):          # locus 0 outermost, locus L - 1 innermost
        w = combo[0][2]
        for l in range(1, L):
            w = w * combo[l][2]
        het = [l for l in range(L) if combo[l][0] != combo[l][1]]
        c = 2.0 if het else 1.0
        phased = het[1:]
        for mask in range(1 << len(phased)):
            A, B = [], []
            for l in range(L):
                lo, hi = combo[l][0], combo[l][1]
                if l in phased and (mask >> phased.index(l)) & 1:
                    A.append(hi); B.append(lo)
                else:
                    A.append(lo); B.append(hi)
            ka = sum(a << (10 * l) for l, a in enumerate(A))
            kb = sum(b << (10 * l) for l, b in enumerate(B))
            out.append((w * c, ka, kb, A, B))
    return out


def brute_count(cands):
    """Distinct unordered haplotype pairs over all combinations, each combination on its own: by brute force over every
    assignment of the two alleles of every locus to the two chromosomes."""
    n = 0
    for combo in itertools.product(*cands):
        seen = set()
        for flips in itertools.product((0, 1), repeat=len(combo)):
            A = tuple(x[f] for x, f in zip(combo, flips))
            B = tuple(x[1 - f] for x, f in zip(combo, flips))
            seen.add((min(A, B), max(A, B)))
        n += len(seen)
    return n


def fit(h1, h2, prob, max_states=4096, min_prob=0.01, maxit=200, tol=1e-8):
    """The whole definition on arrays [L][n][k].  Returns a dict: used, n_states, n_trimmed [n]; keys (ascending), freq [H];
    n_iter, delta, converged, n_zero, loglik; total, prob [n]; hapA, hapB [n, L]; lists (entries per haplotype)."""
    L, n, k = np.shape(h1)
    cand = candidates(h1, h2, prob)
    used = np.zeros(n, bool)
    n_trimmed = np.zeros(n, np.int32)
    n_states = np.zeros(n, np.int64)
    wc, ka, kb, alle, first = [], [], [], [], []
    for s in range(n):
        if any(len(c) == 0 for c in cand[s]):
            continue
        lists, gone = trim(cand[s], min_prob, max_states)
        used[s] = True
        n_trimmed[s] = len(gone)
        st = enumerate_states(lists)
        assert len(st) == closed_count(lists)
        n_states[s] = len(st)
        first.append(len(wc))
        for v, a, b, A, B in st:
            wc.append(v); ka.append(a); kb.append(b); alle.append((A, B))
    if not used.any():
        raise ValueError("no sample used")
    first.append(len(wc))
    n_used = int(used.sum())
    wc = np.array(wc, np.float64)
    entry_key = [None] * (2 * len(wc))
    for s in range(len(wc)):
        entry_key[2 * s], entry_key[2 * s + 1] = ka[s], kb[s]
    keys = sorted(set(entry_key))
    index = {key: i for i, key in enumerate(keys)}
    H = len(keys)
    lists = [[] for _ in range(H)]
    for e, key in enumerate(entry_key):              # ascending entry number
        lists[index[key]].append(e)
    iA = np.array([index[key] for key in ka], np.int64)
    iB = np.array([index[key] for key in kb], np.int64)
    state_of = [np.array(v, np.int64) // 2 for v in lists]

    def e_step(f):
        g = (wc * f[iA]) * f[iB]
        q = np.zeros_like(g)
        tot = np.zeros(n_used)
        for u in range(n_used):
            a, b = first[u], first[u + 1]
            tot[u] = _s64_rows(g[a:b])
            if tot[u] != 0.0:
                q[a:b] = g[a:b] / tot[u]
        return q, tot

    f = np.full(H, 1.0 / H)
    denom = 2.0 * n_used
    n_iter, delta = 0, math.inf
    while n_iter < maxit:
        q, _ = e_step(f)
        fn = np.array([_s64_rows(q[state_of[h]]) / denom for h in range(H)])
        delta = float(np.max(np.abs(fn - f)))
        f = fn
        n_iter += 1
        if delta <= tol:
            break
    q, tot = e_step(f)
    total, pr = np.full(n, np.nan), np.full(n, np.nan)
    hapA, hapB = np.full((n, L), NA, np.int32), np.full((n, L), NA, np.int32)
    for u, s in enumerate(np.flatnonzero(used)):
        a, b = first[u], first[u + 1]
        best = a
        for i in range(a, b):
            if q[i] > q[best]:
                best = i
        total[s], pr[s] = tot[u], q[best]
        hapA[s], hapB[s] = alle[best]
    return dict(used=used, n_states=n_states, n_trimmed=n_trimmed, keys=np.array(keys, np.uint64), freq=f, n_iter=n_iter, delta=delta,
                converged=bool(delta <= tol), n_zero=int(np.count_nonzero(tot == 0.0)),
                loglik=float(sum(math.log(t) for t in tot if t > 0)), total=total, prob=pr, hapA=hapA, hapB=hapB,
                list_lengths=np.array([len(v) for v in lists], np.int64))


# ---- synthetic cohorts ------------------------------------------------------------------------------------------------

def ld_cohort(n, L, k, n_pool, n_allele, seed, p_wrong=0.35):
    """Samples drawn from a pool of `n_pool` haplotypes with skewed frequencies (linkage disequilibrium), and per locus k
    candidate pairs whose first rank is deliberately unreliable: with probability `p_wrong` the true pair is listed second
    behind a decoy.  Returns (truth (lo, hi) [L][n], h1, h2, prob [L][n][k])."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, n_allele, size=(n_pool, L))
    w = rng.dirichlet(np.full(n_pool, 0.6))
    a, b = pool[rng.choice(n_pool, n, p=w)], pool[rng.choice(n_pool, n, p=w)]
    lo, hi = np.minimum(a, b).T, np.maximum(a, b).T                   # [L][n]
    h1 = np.full((L, n, k), NA, np.int32)
    h2 = np.full((L, n, k), NA, np.int32)
    prob = np.zeros((L, n, k))
    for l in range(L):
        for s in range(n):
            pairs = [(int(lo[l, s]), int(hi[l, s]))]
            while len(pairs) < k:
                x, y = sorted(int(v) for v in rng.integers(0, n_allele, 2))
                if (x, y) not in pairs:
                    pairs.append((x, y))
            p = np.sort(rng.dirichlet(np.full(k, 2.0)))[::-1]
            if k > 1 and rng.random() < p_wrong:
                pairs[0], pairs[1] = pairs[1], pairs[0]
                p = np.array([0.5, 0.45] + [0.05 / max(k - 2, 1)] * (k - 2))[:k]
            for r in range(k):
                h1[l, s, r], h2[l, s, r], prob[l, s, r] = pairs[r][0], pairs[r][1], p[r]
    return (lo, hi), h1, h2, prob


def correct_pairs(truth, lo, hi, used=None):
    """Per-locus pairs equal to the truth, summed over loci and (used) samples."""
    ok = (np.asarray(lo) == truth[0]) & (np.asarray(hi) == truth[1])
    return int(ok.sum() if used is None else ok[:, used].sum())
