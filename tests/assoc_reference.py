"""CPU restatement of hlaAssocTest for the tests: DESIGN.md section 20 in numpy, written from the definitions.

``tests_of`` / ``features`` are the tests and their 0/1/2 feature rows, ``labels`` the permuted label rows (selection sampling
on Philox4x32-10 of tests/draws_reference.py), ``chisq_2x2`` / ``chisq_3x2`` the statistics with the stated operation order
(numpy's float64 operations round once each, as the device's do without contraction), ``observed`` / ``permute`` what the
device entries return, ``chisq_p`` / ``fisher_p`` the host p-values and ``assoc_test`` the whole table.  ``Backend``,
``kept_columns``, ``allele_names``, ``gap_partition`` and ``hla_of`` are what the restatements of the other association entries
(tests/assoc*_reference.py) share."""

from __future__ import annotations

import math

import numpy as np

from draws_reference import philox4x32_10

NA_INTEGER = -2147483648
MODELS = ("dominant", "additive", "recessive", "genotype")


def kept(a1, a2, y):
    """The samples with two known alleles, in order: their alleles and labels."""
    a1, a2, y = np.asarray(a1, np.int64), np.asarray(a2, np.int64), np.asarray(y, np.int64)
    ok = (a1 != NA_INTEGER) & (a2 != NA_INTEGER)
    return a1[ok], a2[ok], y[ok]


def tests_of(n_allele, group_of=None):
    """(table [1 + n_part, n_allele] with the identity partition first, part [T], level [T]): one test per allele, then one
    per level 0 .. max id of every partition."""
    rows = [np.arange(n_allele, dtype=np.int64)]
    part, lev = [0] * n_allele, list(range(n_allele))
    if group_of is not None:
        for q, g in enumerate(np.asarray(group_of, np.int64).reshape(-1, n_allele)):
            rows.append(g)
            part += [q + 1] * (int(g.max()) + 1)
            lev += list(range(int(g.max()) + 1))
    return np.stack(rows), np.array(part), np.array(lev)


def features(a1, a2, table, part, lev, model):
    """int64 [rows, n] over the kept samples: d >= 1, d, d == 2 with d the number of the sample's alleles in the level;
    ``genotype``: rows 2t (d == 1) and 2t + 1 (d == 2)."""
    d = (table[part][:, a1] == lev[:, None]).astype(np.int64) + (table[part][:, a2] == lev[:, None])
    if model == "dominant":
        return (d >= 1).astype(np.int64)
    if model == "additive":
        return d
    if model == "recessive":
        return (d == 2).astype(np.int64)
    out = np.empty((2 * len(part), len(a1)), np.int64)
    out[0::2], out[1::2] = d == 1, d == 2
    return out


def labels(seed, perm0, n_perm, n, n_case):
    """uint8 [n_perm, n]: row j is permutation perm0 + j.  Sample i is a case iff u * (n - i) < need << 32 with u word
    i & 3 of Philox4x32-10(counter (i >> 2, 0, p lo, p hi), key (seed lo, seed hi)); need starts at n_case."""
    seed = int(seed)
    p = [int(perm0) + j for j in range(n_perm)]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    plo = np.array([v & 0xFFFFFFFF for v in p], np.uint64)
    phi = np.array([v >> 32 for v in p], np.uint64)
    need = np.full(n_perm, n_case, np.uint64)
    out = np.zeros((n_perm, n), np.uint8)
    w = None
    for i in range(n):
        if i & 3 == 0:
            counter = np.stack([np.full(n_perm, i >> 2, np.uint64), np.zeros(n_perm, np.uint64), plo, phi], axis=-1)
            w = philox4x32_10(counter, key).astype(np.uint64)
        case = w[:, i & 3] * np.uint64(n - i) < (need << np.uint64(32))
        need = need - case.astype(np.uint64)
        out[:, i] = case
    return out


def chisq_2x2(N, a, r1, c1):
    """Yates-corrected chi-square from a = case carriers (any shape), r1 = carriers (broadcasts), c1 = cases, N = units."""
    a, r1 = np.asarray(a, np.int64), np.asarray(r1, np.int64)
    N, c1 = np.int64(N), np.int64(c1)
    r2, c2 = N - r1, N - c1
    det = N * a - r1 * c1
    D = 2 * np.abs(det) - N
    d = D.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        st = ((d * d) * np.float64(N)) / ((4.0 * (r1 * r2).astype(np.float64)) * np.float64(c1 * c2))
    st = np.where(D <= 0, 0.0, st)
    empty = (r1 == 0) | (r2 == 0) | (c1 == 0) | (c2 == 0)
    return np.where(empty, np.nan, st)


def chisq_3x2(N, c1, r_het, r_hom, x_het, x_hom):
    """Uncorrected chi-square of rows none / het / hom x columns control / case, the six terms added in that order."""
    r_het, r_hom, x_het, x_hom = (np.asarray(v, np.int64) for v in (r_het, r_hom, x_het, x_hom))
    N, c1 = np.int64(N), np.int64(c1)
    c0 = N - c1
    r_non = N - r_het - r_hom
    x_non = c1 - x_het - x_hom
    s = None
    with np.errstate(divide="ignore", invalid="ignore"):
        for r, x in ((r_non, x_non), (r_het, x_het), (r_hom, x_hom)):
            for c, cell in ((c0, r - x), (c1, x)):
                num = (N * cell - r * c).astype(np.float64)
                term = (num * num) / (np.float64(N) * (r * c).astype(np.float64))
                s = term if s is None else s + term
    empty = (r_non == 0) | (r_het == 0) | (r_hom == 0) | (c0 == 0) | (c1 == 0)
    return np.where(empty, np.nan, s)


def _stats(model, F, rsum, L, n, n_case):
    """Statistics [T, n_lab] of the label rows L [n_lab, n] (and the case-carrier counts [rows, n_lab])."""
    x = F @ L.T.astype(np.int64)
    if model == "genotype":
        st = chisq_3x2(n, n_case, rsum[0::2, None], rsum[1::2, None], x[0::2], x[1::2])
    else:
        unit = 2 if model == "additive" else 1
        st = chisq_2x2(unit * n, x, rsum[:, None], unit * n_case)
    return st, x


def max_and_count(st, stat):
    """(max_stat [n_perm], count_point int64 [T]) of the permuted statistics st [T, n_perm] against the observed stat [T]: the
    largest statistic of every permutation (NaN where all are NaN) and, per test, the permutations with st >= stat."""
    best = np.where(np.isnan(st), -1.0, st).max(axis=0) if len(st) else np.full(st.shape[1], -1.0)
    with np.errstate(invalid="ignore"):
        count = (st >= stat[:, None]).sum(axis=1).astype(np.int64)
    return np.where(best < 0, np.nan, best), count


class Analysis:
    """The tests of one cohort: ``a1``, ``a2`` (NA_INTEGER = unknown), ``y`` 0 / 1, as hibag_hip_assoc_new takes them."""

    def __init__(self, a1, a2, y, n_allele, group_of, model):
        self.model = model
        self.a1, self.a2, self.y = kept(a1, a2, y)
        self.n, self.n_case = len(self.y), int(self.y.sum())
        self.table, self.part, self.lev = tests_of(n_allele, group_of)
        self.F = features(self.a1, self.a2, self.table, self.part, self.lev, model)
        self.rsum = self.F.sum(axis=1)
        self.n_tests = len(self.part)
        st, x = _stats(model, self.F, self.rsum, self.y[None, :], self.n, self.n_case)
        self.stat = st[:, 0]
        x = x[:, 0]
        unit = 2 if model == "additive" else 1
        N, c1 = unit * self.n, unit * self.n_case
        tab = np.zeros((self.n_tests, 6), np.int64)
        if model == "genotype":
            r_het, r_hom, x_het, x_hom = self.rsum[0::2], self.rsum[1::2], x[0::2], x[1::2]
            x_non = c1 - x_het - x_hom
            tab[:, 0], tab[:, 1] = (N - r_het - r_hom) - x_non, x_non
            tab[:, 2], tab[:, 3] = r_het - x_het, x_het
            tab[:, 4], tab[:, 5] = r_hom - x_hom, x_hom
        else:
            tab[:, 0], tab[:, 1] = (N - self.rsum) - (c1 - x), c1 - x
            tab[:, 2], tab[:, 3] = self.rsum - x, x
        self.tab = tab

    def labels(self, seed, perm0, n_perm):
        return labels(seed, perm0, n_perm, self.n, self.n_case)

    def permute(self, seed, perm0, n_perm):
        """(max_stat [n_perm], count_point int64 [T]) of permutations perm0 .. perm0 + n_perm - 1."""
        st, _ = _stats(self.model, self.F, self.rsum, self.labels(seed, perm0, n_perm), self.n, self.n_case)
        return max_and_count(st, self.stat)


class Backend:
    """The cohort behind the interface every ``_backend`` seam of hibag_amd's association entries drives; a restatement adds
    its entry's methods."""

    dtype = np.float64

    def __init__(self, a1, a2, y, n_allele, group_of, model):
        self.model = MODELS[model]
        self.A = Analysis(a1, a2, y, n_allele, group_of, self.model)
        self.n_tests, self.n_kept = self.A.n_tests, self.A.n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def feature_rows(self, row0, n_rows):
        return self.A.F[row0:row0 + n_rows].astype(np.int8)


def kept_columns(a1, a2, *columns):
    """The columns (last axis = samples) restricted to the samples with two known alleles."""
    ok = (np.asarray(a1) != NA_INTEGER) & (np.asarray(a2) != NA_INTEGER)
    return [np.ascontiguousarray(np.asarray(c)[..., ok]) for c in columns]


def allele_names(n_allele):
    return [f"{k + 1:02d}:01" for k in range(n_allele)]        # (sorted order = index order)


def gap_partition(n_allele):
    """group_of [1, n_allele] of one partition whose level 1 is empty (levels 0, 2, 3 are in use)."""
    return np.where(np.arange(n_allele) % 3 == 0, 0, 2 + np.arange(n_allele) % 2)[None, :].astype(np.int32)


def hla_of(a1, a2, prob, n_allele, gap=None, locus="A"):
    """(hla, names, groups or None): the cohort of allele indices as the entries take it, the alleles under ``allele_names``;
    ``gap``: a ``gap_partition`` as the groups ``pos``, which name one level more than the partition has."""
    import hibag_amd as hb
    names = allele_names(n_allele)
    hla = hb.HlaAlleleClass(locus=locus, sample_id=[f"s{i}" for i in range(len(a1))], allele1=[None if a < 0 else names[a] for a in a1],
                            allele2=[None if a < 0 else names[a] for a in a2], prob=prob)
    return hla, names, None if gap is None else hb.HlaAlleleGroups(names, ["pos"], [["x", "gap", "y", "z", "beyond"]], gap)


def chisq_p(st, df):
    if math.isnan(st):
        return math.nan
    return math.erfc(math.sqrt(st / 2.0)) if df == 1 else math.exp(-st / 2.0)


def fisher_p(x00, x01, x10, x11):
    """Two-sided exact test of the 2 x 2 table rows (without, with) x columns (control, case) with R's rule: the sum of the
    probabilities of the tables whose probability is <= observed * (1 + 1e-7), margins fixed; log probabilities from
    lgamma, scaled by the largest, added one by one along the support.  NaN with an empty margin."""
    r1, r2, c1 = x10 + x11, x00 + x01, x01 + x11
    N = r1 + r2
    c2 = N - c1
    if 0 in (r1, r2, c1, c2):
        return math.nan

    def lf(v):
        return math.lgamma(v + 1.0)

    lo, hi = max(0, c1 - r2), min(r1, c1)
    logd = np.array([((lf(r1) - lf(k) - lf(r1 - k)) + (lf(r2) - lf(c1 - k) - lf(r2 - c1 + k))) - (lf(N) - lf(c1) - lf(c2))
                     for k in range(lo, hi + 1)])
    d = np.exp(logd - logd.max())
    limit = d[x11 - lo] * (1.0 + 1e-7)
    tail = total = 0.0
    for v in d:
        total = total + v
        if v <= limit:
            tail = tail + v
    return float(tail / total)


def assoc_test(a1, a2, y, n_allele, group_of, model, n_perm=0, seed=0):
    """Every column of hlaAssocTest for tests the device knows: dict of arrays in test order."""
    A = Analysis(a1, a2, y, n_allele, group_of, model)
    k = 3 if model == "genotype" else 2
    cells = A.tab.reshape(-1, 3, 2)[:, :k]
    counts = cells[:, :, 0] + cells[:, :, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = np.round(100.0 * (cells[:, :, 1] / counts), 1)
    pct[counts == 0] = np.nan
    out = {"counts": counts, "pct": pct, "chisq_st": A.stat, "table": A.tab,
           "chisq_p": np.array([chisq_p(s, 2 if model == "genotype" else 1) for s in A.stat]),
           "fisher_p": np.array([math.nan if model == "genotype" else fisher_p(*row[:4]) for row in A.tab.tolist()])}
    if n_perm > 0:
        max_stat, count = A.permute(seed, 1, n_perm)
        with np.errstate(invalid="ignore"):
            count_max = (max_stat[None, :] >= A.stat[:, None]).sum(axis=1)
        nan = np.isnan(A.stat)
        out["max_stat"] = max_stat
        out["perm_p"] = np.where(nan, np.nan, (1 + count) / (n_perm + 1))
        out["perm_p_adj"] = np.where(nan, np.nan, (1 + count_max) / (n_perm + 1))
    return out
