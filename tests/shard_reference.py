"""Classifier-sharded prediction restated on the host: the partial sums of a run of classifiers, their merge, the finish.

The sharded route (hibag_amd/csrc/hibag_shard.hip) is a fixed sequence of IEEE additions wherever the order of the merge is
defined: a shard adds its classifiers' terms in classifier order from +0.0, shards that share a device are added in shard
order (k_add_partial), a one-rank all-reduce is the identity and a two-rank one adds two numbers, which commutes.  So the
device's sums can be replayed exactly, and the finish (hibag_amd/csrc/hibag_k_finish.h: finish_call, finish_dosage,
k_finish_prob) is a pure function of the merged sums.  numpy and oracle/oracle.py only: nothing of hibag_amd's kernels.

    partial_sums   [P + 3, n_pad] of classifiers lo .. hi-1, as hibag_hip_predict_partial_device defines them
    merge          left to right, in shard order
    merge_by_rank  per distinct device in shard order, then the (at most two) per-device sums
    finish         the six PredictHLA outputs from merged sums
    assert_same    every entry of every key equal in its bits (NaN equal to NaN)
"""

from __future__ import annotations

import numpy as np

NA_INTEGER = -2147483648
KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")
FIN_SEG = 16                      # hibag_k_finish.h: segments of the cell range in finish_call


def n_pad_of(n: int) -> int:
    return (n + 63) // 64 * 64


def snp_counts(model) -> np.ndarray:
    """Classifiers using each SNP, over the FULL model (``_GetSNPWeights``, src/LibHLA.cpp:2484-2496)."""
    sw = np.zeros(model.n_snp, np.int64)
    for c in model.classifiers:
        np.add.at(sw, c.snpidx, 1)
    return sw


def classifier_weights(model, G) -> np.ndarray:
    """w_c of every (classifier, sample), [C, n]: the typed share of the classifier's SNP counts (src/LibHLA.cpp:2418-2431)."""
    sw = snp_counts(model)
    W = np.zeros((len(model.classifiers), G.shape[0]))
    for c, cl in enumerate(model.classifiers):
        cnt = sw[cl.snpidx]
        tot = int(cnt.sum())
        for i in range(G.shape[0]):
            g = G[i][cl.snpidx]
            ok = (g >= 0) & (g <= 2)
            W[c, i] = float(int(cnt[ok].sum())) / tot if tot > 0 else 0.0
    return W


def partial_sums(O, fm, model, lo, hi, G) -> np.ndarray:
    """float64 [P + 3, n_pad], n_pad = n rounded up to 64, of classifiers lo .. hi-1 of `model` (`fm` = O.flatten(model)):
    rows 0..P-1  S[p] += prob_c[p] * w_c, classifiers in order from +0.0, those with w_c <= 0 passed over;
    row P sum w_c, row P + 1 sum total_c * w_c, row P + 2 sum w_c.  Columns n .. n_pad-1 are zero (the device's are
    whatever its padding lanes computed: never compared)."""
    P = fm.n_hla * (fm.n_hla + 1) // 2
    n = G.shape[0]
    sw = snp_counts(model)
    part = np.zeros((P + 3, n_pad_of(n)))
    for i in range(n):
        for c in range(lo, hi):
            cl = model.classifiers[c]
            g = G[i][cl.snpidx]
            ok = (g >= 0) & (g <= 2)
            tot = int(sw[cl.snpidx].sum())
            w = float(int(sw[cl.snpidx][ok].sum())) / tot if tot > 0 else 0.0
            if w <= 0:
                continue
            s1, s2 = O.int_to_snp(G[i], cl.snpidx)
            prob, total = O.post_prob2(fm, c, s1, s2)
            part[:P, i] += prob * w
            part[P, i] += w
            part[P + 1, i] += total * w
            part[P + 2, i] += w
    return part


def merge(parts) -> np.ndarray:
    """parts[0] + parts[1] + ... left to right: shards that share a device (k_add_partial, in shard order)."""
    parts = list(parts)
    if not parts:
        raise ValueError("nothing to merge")
    out = np.array(parts[0], np.float64, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in parts[1:]:
            out = out + p
    return out


def merge_by_rank(parts, devices) -> np.ndarray:
    """One rank per distinct device, in the order the devices first appear: each rank's shards in shard order, then the
    ranks' sums.  Two addends commute, so up to two ranks are defined in their bits; a ring over more is not."""
    parts, devices = list(parts), list(devices)
    if len(parts) != len(devices):
        raise ValueError("one device per shard")
    order = []
    for d in devices:
        if d not in order:
            order.append(d)
    if len(order) > 2:
        raise ValueError(f"{len(order)} ranks: the order of an all-reduce over more than two is not specified")
    return merge([merge([p for p, d in zip(parts, devices) if d == r]) for r in order])


def cell_pairs(n_hla: int):
    """(h1, h2) of every cell, p = h2 + h1 (2 n - h1 - 1) / 2 (src/LibHLA.cpp:1523)."""
    h1 = np.repeat(np.arange(n_hla), np.arange(n_hla, 0, -1)).astype(np.int32)
    h2 = np.concatenate([np.arange(i, n_hla) for i in range(n_hla)]).astype(np.int32)
    return h1, h2


def finish(merged, n_hla: int, n: int) -> dict:
    """hibag_k_finish.h replayed: x = v * (1 / sum_w) where sum_w > 0, else v; the call is the first strict maximum of x in
    cell order from best = 0 (NA and prob 0.0 when nothing is positive); matching = row P + 1 / row P + 2; dosage[h] adds
    (0,h), (1,h), ..., 2 (h,h), (h,h+1), ... in that order; postprob[s][p] = x.  A NaN sum_w: NA call, NaN prob, dosage
    and postprob."""
    P = n_hla * (n_hla + 1) // 2
    M = np.asarray(merged, np.float64)
    if M.ndim != 2 or M.shape[0] != P + 3 or M.shape[1] < n:
        raise ValueError(f"merged sums must be [{P + 3}, >= {n}]")
    M = M[:, :n]
    sum_w = M[P]
    poisoned = np.isnan(sum_w)
    scale = sum_w > 0
    with np.errstate(all="ignore"):
        ff = 1.0 / sum_w
        X = np.where(scale, M[:P] * ff, M[:P])
        matching = M[P + 1] / M[P + 2]
    best = np.zeros(n)
    cell = np.full(n, -1, np.int64)
    for p in range(P):
        win = best < X[p]
        best = np.where(win, X[p], best)
        cell[win] = p
    cell[poisoned] = -1
    best = np.where(poisoned, sum_w, best)
    c1, c2 = cell_pairs(n_hla)
    called = cell >= 0
    h1 = np.where(called, c1[np.maximum(cell, 0)], NA_INTEGER).astype(np.int32)
    h2 = np.where(called, c2[np.maximum(cell, 0)], NA_INTEGER).astype(np.int32)
    prob = np.where(called | poisoned, best, 0.0)
    dosage = np.zeros((n, n_hla))
    with np.errstate(all="ignore"):
        for h in range(n_hla):
            d = np.zeros(n)
            for g in range(n_hla):
                a, b = (g, h) if g < h else (h, g)
                x = X[b + a * (2 * n_hla - a - 1) // 2]
                d = d + (2 * x if g == h else x)
            dosage[:, h] = np.where(poisoned, sum_w, d)
    postprob = np.where(poisoned[None, :], sum_w[None, :], X).T.copy()
    return dict(h1=h1, h2=h2, prob=prob, matching=matching, dosage=dosage, postprob=postprob)


def _differs(a, b):
    if a.dtype.kind == "f":
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        return ~same
    return a != b


def assert_same(got, want, keys=None, what=""):
    """Every entry of every key of `want` (or of `keys`) equal in its bits, NaN equal to NaN; the message names the first
    differing key, its first sample and that sample's 64-sample group."""
    for k in (keys if keys is not None else [k for k in KEYS if k in want]):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        bad = _differs(a, b)
        if not bad.any():
            continue
        rows = np.flatnonzero(bad.reshape(len(a), -1).any(axis=1))
        s = int(rows[0])
        raise AssertionError(f"{what} {k}: {len(rows)} samples differ, the first is sample {s} (group {s // 64}): "
                             f"got {a[s]!r}, reference {b[s]!r}; groups {sorted(set((rows // 64).tolist()))[:20]}")


def assert_same_rows(got, want, what=""):
    """Partial sums [rows, n]: equal in their bits (NaN equal to NaN); names the first differing row, sample and group."""
    a, b = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = _differs(a, b)
    if not bad.any():
        return
    r, s = (int(v) for v in np.argwhere(bad)[0])
    cols = np.flatnonzero(bad.any(axis=0))
    raise AssertionError(f"{what} partial sums: {int(bad.sum())} entries differ, the first is row {r} of {a.shape[0]}, sample {s} "
                         f"(group {s // 64}): got {a[r, s]!r}, reference {b[r, s]!r}; groups {sorted(set((cols // 64).tolist()))[:20]}")


# ---- planted merged sums for the finish kernels --------------------------------------------------------------------
# One column = one sample.  Every planter takes (rng, n_hla) and returns a [P + 3] column or None where the shape has no
# room for the property; tests/test_shard_host.py asserts the property of each on the host's finish.

def _random_column(rng, P, sum_w=None):
    col = np.empty(P + 3)
    col[:P] = rng.uniform(0.01, 1.0, P)
    col[P] = rng.uniform(0.5, 40.0) if sum_w is None else sum_w
    col[P + 1] = rng.uniform(1e-9, 1e-3)
    col[P + 2] = col[P]
    return col


def segments(P: int):
    """finish_call's cell ranges: FIN_SEG segments of per = ceil(P / FIN_SEG) cells."""
    per = (P + FIN_SEG - 1) // FIN_SEG
    return per, [(g * per, min(P, g * per + per)) for g in range(FIN_SEG)]


def _tie(rng, P, first, later):
    col = _random_column(rng, P)
    col[first] = col[later] = 2.5
    return col


def plant_tie_same_block(rng, n_hla):
    """The maximum again in a later cell of the same eight-wide block of a segment."""
    P = n_hla * (n_hla + 1) // 2
    per, segs = segments(P)
    if per < 8:
        return None
    lo = segs[1][0]
    return _tie(rng, P, lo + 2, lo + 6)


def plant_tie_next_block(rng, n_hla):
    """The maximum again behind the first eight-wide block of the same segment (its next block, or its tail)."""
    P = n_hla * (n_hla + 1) // 2
    per, segs = segments(P)
    lo, hi = segs[1]
    if hi - lo < 9:
        return None
    return _tie(rng, P, lo + 3, lo + 9 if hi - lo >= 16 else hi - 1)


def plant_tie_tail(rng, n_hla):
    """The maximum twice among the cells a segment scans one by one (fewer than eight left)."""
    P = n_hla * (n_hla + 1) // 2
    per, segs = segments(P)
    lo, hi = segs[0]
    t0 = lo + (hi - lo) // 8 * 8
    if hi - t0 < 2:
        return None
    return _tie(rng, P, t0, hi - 1)


def plant_tie_later_segment(rng, n_hla):
    """The maximum again in a later segment: the merge of the segments must keep the first."""
    P = n_hla * (n_hla + 1) // 2
    per, segs = segments(P)
    live = [g for g, (lo, hi) in enumerate(segs) if hi > lo]
    if len(live) < 2:
        return None
    return _tie(rng, P, segs[live[0]][1] - 1, segs[live[-1]][0])


def plant_scaled_tie(rng, n_hla):
    """Two neighbouring doubles, the smaller first, whose products with ff = 1 / sum_w are equal: the scaled values tie, so
    the FIRST cell is called although the second holds the larger sum."""
    P = n_hla * (n_hla + 1) // 2
    if P < 2:
        return None
    sum_w = 3.0
    ff = 1.0 / sum_w
    while True:
        a = rng.uniform(2.0, 4.0)
        b = np.nextafter(a, np.inf)
        if a * ff == b * ff:
            break
    col = _random_column(rng, P, sum_w)
    col[0], col[1] = a, b
    return col


def plant_zero_weight_positive(rng, n_hla):
    """sum_w = 0 with positive cells: nothing is scaled, the raw sums come back."""
    P = n_hla * (n_hla + 1) // 2
    col = _random_column(rng, P, 0.0)
    col[P + 2] = 0.0
    return col


def plant_zero_weight_zero(rng, n_hla):
    """sum_w = 0 and every cell zero (a sample no classifier was used for): NA call, prob 0.0, matching 0 / 0."""
    P = n_hla * (n_hla + 1) // 2
    return np.zeros(P + 3)


def plant_nan_weight(rng, n_hla):
    """sum_w = NaN (the mark of a failed hand-over) over finite rows: NA call, NaN prob, dosage and postprob; matching is
    still the quotient of its two rows."""
    P = n_hla * (n_hla + 1) // 2
    col = _random_column(rng, P)
    col[P] = np.nan
    return col


def plant_nan_before_max(rng, n_hla):
    """A NaN cell ahead of the maximum: no comparison with it is true, the maximum is still found."""
    P = n_hla * (n_hla + 1) // 2
    if P < 2:
        return None
    col = _random_column(rng, P)
    col[0] = np.nan
    col[P - 1] = 3.0
    return col


def plant_nan_only(rng, n_hla):
    """A NaN cell as the only non-zero one: NA call, prob 0.0."""
    P = n_hla * (n_hla + 1) // 2
    col = _random_column(rng, P)
    col[:P] = 0.0
    col[P // 2] = np.nan
    return col


def plant_inf_twice(rng, n_hla):
    """+inf in two cells: the first wins."""
    P = n_hla * (n_hla + 1) // 2
    if P < 2:
        return None
    col = _random_column(rng, P)
    col[P // 3] = col[P - 1] = np.inf
    return col


def plant_subnormal_cells(rng, n_hla):
    """Subnormal cells under a large sum_w: every product rounds to zero, so NA call and prob 0.0."""
    P = n_hla * (n_hla + 1) // 2
    col = _random_column(rng, P, 1e6)
    col[:P] = rng.integers(1, 1000, P) * 5e-324
    return col


def plant_subnormal_weight(rng, n_hla):
    """A subnormal sum_w: ff = 1 / sum_w = inf, every positive cell becomes inf and the first one is called."""
    P = n_hla * (n_hla + 1) // 2
    col = _random_column(rng, P, 1e-310)
    col[P + 2] = 1e-310
    return col


PLANTS = (plant_tie_same_block, plant_tie_next_block, plant_tie_tail, plant_tie_later_segment, plant_scaled_tie,
          plant_zero_weight_positive, plant_zero_weight_zero, plant_nan_weight, plant_nan_before_max, plant_nan_only,
          plant_inf_twice, plant_subnormal_cells, plant_subnormal_weight)


def planted_sums(n_hla: int, seed: int = 0):
    """([P + 3, k] planted columns, their planters' names) of every property the shape has room for."""
    rng = np.random.default_rng(9000 + 31 * n_hla + seed)
    cols, names = [], []
    for f in PLANTS:
        col = f(rng, n_hla)
        if col is not None:
            cols.append(col)
            names.append(f.__name__)
    return np.stack(cols, axis=1), names


def synthetic_merged(n_hla: int, n: int, seed: int = 0):
    """The finish kernels' test input: float64 [P + 3, n_pad] of random positive columns, and among them the planted ones:
    with k planted columns, column s holds planted column (s % 64) % (k + 8) where that is below k -- every 64-sample group, the
    ragged last one included (whose last column stays random), sees planted and random columns side by side (n = 1 has
    room for the first only: the others go one call at a time, :func:`planted_sums`).  Returns (sums, {column: planter's name})."""
    P = n_hla * (n_hla + 1) // 2
    rng = np.random.default_rng(7000 + 131 * n_hla + n + seed)
    out = np.zeros((P + 3, n_pad_of(n)))
    for s in range(n_pad_of(n)):
        out[:, s] = _random_column(rng, P)
    planted, names = planted_sums(n_hla, seed)
    k = planted.shape[1]
    where = {}
    for s in range(n):
        j = (s % 64) % (k + 8)
        if j < k and (s < n - 1 or n == 1):
            out[:, s] = planted[:, j]
            where[s] = names[j]
    return out, where


# ---- the hand-built case of tests/test_hip_shard.py and tests/test_shard_host.py ---------------------------------------
# (the model's containers are hibag_amd.model's plain dataclasses, which hlaModelFromObj insists on: no kernel is involved)

HAND_WIDTHS = (3, 14, 28, 29, 31, 32, 33, 60, 100, 112, 113, 128)
HAND_EMPTY_AT = 6                 # the classifier without haplotypes: index 6 of 13, on two SNPs of its own
HAND_SNPS = 142
HAND_SKIPPED = (0, 3)             # classifiers samples 64..66 miss every SNP of
HAND_GROUP_SKIPPED = 4            # the classifier every sample of the second group misses every SNP of
HAND_USE_EMPTY = (10, 11, 12, 70, 71, 129)       # the samples typed at the empty classifier's SNPs: NaN in every cell


def hand_model(seed: int = 4242, n_hla: int = 5, widths=HAND_WIDTHS, empty_at=HAND_EMPTY_AT):
    """(model, founders): `n_hla` alleles, one classifier per entry of `widths` over SNPs 0..139 -- 8 to 40 haplotypes,
    every allele with at least one, families of 1-3 flipped sites around the allele's founder -- and, at `empty_at`
    (None: left out), one classifier without haplotypes on SNPs 140 and 141.  With the default widths every distance
    engine occurs: FP4 in one step (3, 14, 28, 29), int8 (31, 32), FP4 in several steps (33 .. 112), VALU (113, 128)."""
    from hibag_amd.model import Classifier, HlaAttrBagObj
    rng = np.random.default_rng(seed)
    S = HAND_SNPS
    founders = (rng.random((n_hla, S)) < rng.uniform(0.15, 0.85, S)).astype(np.uint8)
    classifiers = []
    for k in widths:
        snpidx = rng.choice(S - 2, size=k, replace=False).astype(np.int32)
        H = int(rng.integers(8, 41))
        hla = np.sort(np.concatenate([np.arange(n_hla), rng.integers(0, n_hla, H - n_hla)])).astype(np.int32)
        rows, seen = [], set()
        for a in hla:
            h = founders[a, snpidx].copy()
            if int(a) in seen:
                flips = rng.choice(k, size=min(k, int(rng.integers(1, 4))), replace=False)
                h[flips] ^= 1
            seen.add(int(a))
            rows.append("".join("1" if b else "0" for b in h))
        freq = rng.gamma(0.5, 1.0, H) + 1e-5
        classifiers.append(Classifier(snpidx=snpidx, freq=freq / freq.sum(), hla=hla, haplo=rows))
    if empty_at is not None:
        classifiers.insert(empty_at, Classifier(snpidx=np.array([S - 2, S - 1]), freq=np.zeros(0), hla=np.zeros(0, np.int32), haplo=[]))
    model = HlaAttrBagObj(n_samp=0, n_snp=S, hla_allele=[f"{a + 1:02d}" for a in range(n_hla)], classifiers=classifiers)
    return model, founders


def hand_samples(model, founders, n: int = 130, seed: int = 4243, structured: bool = True):
    """int32 [n, n_snp]: two founders per sample, 0.2 % genotyping errors, 3 % missing; with `structured` (the 13-classifier
    model, n = 130): sample 5 all missing, samples 64..66 missing every SNP of classifiers HAND_SKIPPED, the second
    64-sample group missing every SNP of classifier HAND_GROUP_SKIPPED, and the empty classifier's two SNPs typed for
    HAND_USE_EMPTY only."""
    rng = np.random.default_rng(seed)
    n_hla, S = founders.shape
    a = rng.integers(0, n_hla, (n, 2))
    g = founders[a[:, 0]].astype(np.int32) + founders[a[:, 1]].astype(np.int32)
    e = rng.random((n, S)) < 0.002
    g = np.where(e, (g + rng.integers(1, 3, (n, S))) % 3, g).astype(np.int32)
    g[rng.random((n, S)) < 0.03] = NA_INTEGER
    if structured:
        snps = [np.asarray(c.snpidx) for c in model.classifiers]
        typed = g[:, S - 2:].copy()
        g[:, S - 2:] = NA_INTEGER
        for s in HAND_USE_EMPTY:
            g[s, S - 2:] = np.where(typed[s] == NA_INTEGER, 1, typed[s])
        for c in HAND_SKIPPED:
            g[np.ix_(range(64, 67), snps[c])] = NA_INTEGER
        g[np.ix_(range(64, 128), snps[HAND_GROUP_SKIPPED])] = NA_INTEGER
        g[5, :] = NA_INTEGER
    return np.ascontiguousarray(g)


def shard_bounds(n: int, world: int, rank: int):
    """hibag_hip_shard_bounds on the host: [lo, hi) of shard `rank` of `world` (sizes differ by at most one)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_parts(O, fm, model, world: int, G):
    """partial_sums of every shard of `world`."""
    C = len(model.classifiers)
    return [partial_sums(O, fm, model, *shard_bounds(C, world, r), G) for r in range(world)]
