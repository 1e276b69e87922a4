"""CPU restatement of hlaAssocHaplo for the tests, in plain Python and numpy, written from the
definitions and independent of hibag_amd/assochaplo.py and of the device code.

``dosages`` is the posterior haplotype dosage (section 29 item 7) on top of tests/haplo_reference.py's ``fit``: the states are
enumerated again, the last E step is made under the fit's frequencies with the summation rule S64, and every dosage is the
sequential sum written out.  ``RealScore`` is the score test on real-valued rows on top of tests/assocscore_reference.py's
``Score`` (dtype-generic, as that is); ``Backend`` puts it behind the interface ``hibag_amd.assochaplo`` drives;
``haplo_result`` is an ``HlaHaplotypeResult`` made of the restatement's numbers, so that ``hlaAssocHaplo`` runs without a
device.  ``real_case`` are the rows, sets and replicates of the device comparisons."""

from __future__ import annotations

import numpy as np

import assocscore_reference as SR
import haplo_reference as R

NA = R.NA


# ---- the dosage ---------------------------------------------------------------------------------------------------------
def dosages(h1, h2, prob, max_states=4096, min_prob=0.01, maxit=200, tol=1e-8):
    """``R.fit`` of the same arguments, plus ``D`` float64 [H][n] in ascending-key order, ``q`` (the last E step's posteriors,
    all states of the used samples back to back), ``first`` (the used samples' first states) and ``lists`` (per haplotype its
    entries in ascending number)."""
    L, n, k = np.shape(h1)
    out = R.fit(h1, h2, prob, max_states=max_states, min_prob=min_prob, maxit=maxit, tol=tol)
    cand = R.candidates(h1, h2, prob)
    wc, ka, kb, first = [], [], [], []
    for s in range(n):
        if not out["used"][s]:
            continue
        lists, _ = R.trim(cand[s], min_prob, max_states)
        first.append(len(wc))
        for v, a, b, _, _ in R.enumerate_states(lists):
            wc.append(v); ka.append(a); kb.append(b)
    first.append(len(wc))
    keys = [int(x) for x in out["keys"]]
    index = {key: i for i, key in enumerate(keys)}
    f = out["freq"]
    q = [0.0] * len(wc)
    for u in range(len(first) - 1):
        a, b = first[u], first[u + 1]
        g = [(wc[s] * float(f[index[ka[s]]])) * float(f[index[kb[s]]]) for s in range(a, b)]
        tot = R.s64(g)
        for s in range(a, b):
            q[s] = g[s - a] / tot if tot != 0.0 else 0.0
    lists = [[] for _ in keys]
    for s in range(len(wc)):                       # ascending entry number: 2 s, then 2 s + 1
        lists[index[ka[s]]].append(2 * s)
        lists[index[kb[s]]].append(2 * s + 1)
    sample_of = np.zeros(len(wc), np.int64)
    used = np.flatnonzero(out["used"])
    for u in range(len(first) - 1):
        sample_of[first[u]:first[u + 1]] = used[u]
    D = np.zeros((len(keys), n))
    D[:, ~out["used"]] = np.nan
    for h, entries in enumerate(lists):
        acc = {}
        for e in entries:
            i = int(sample_of[e // 2])
            acc[i] = acc.get(i, 0.0) + q[e // 2]
        for i, v in acc.items():
            D[h, i] = v
    return dict(out, D=D, q=np.array(q), first=first, lists=lists, sample_of=sample_of)


def haplo_result(h1, h2, prob, n_allele, dosage_min_freq=None, **kw):
    """The restatement's numbers as the ``HlaHaplotypeResult`` that ``hlaHaplotypes`` returns for the same candidates (levels
    ``L<l>*<index>``, sample ids ``s<i>``)."""
    from hibag_amd import haplo
    L, n, _ = np.shape(h1)
    r = dosages(h1, h2, prob, **kw)
    order = np.lexsort((r["keys"], -r["freq"]))
    levels = [[f"L{l}*{i:04d}" for i in range(n_allele)] for l in range(L)]
    res = haplo.HlaHaplotypeResult([f"L{l}" for l in range(L)], levels, [f"s{i}" for i in range(n)], haplo.decode_keys(r["keys"][order], L),
                                   r["freq"][order], r["keys"][order], r["n_iter"], r["converged"], r["delta"], r["loglik"], r["n_zero"],
                                   r["hapA"], r["hapB"], r["prob"], r["used"], r["total"], r["n_states"], r["n_trimmed"],
                                   (np.asarray(h1)[:, :, 0].copy(), np.asarray(h2)[:, :, 0].copy()))
    if dosage_min_freq is not None:
        idx = np.flatnonzero(r["freq"][order] >= dosage_min_freq)
        res.dosage_min_freq, res.dosage_index, res.dosage = float(dosage_min_freq), idx, r["D"][order[idx]]
    return res, r


# ---- the score test on real rows --------------------------------------------------------------------------------------
class RealScore(SR.Score):
    """``Score`` with the real-valued rows X [rows, n] in place of the int8 features: items 4 and 7 of section 28 with X for F;
    a row is dropped when S_jj == 0 (in place of "row sum 0")."""

    def __init__(self, X, y, covar=None, weight=None, maxit=25, epsilon=1e-8, dtype=np.float64):
        X = np.asarray(X, np.float64)
        super().__init__(np.zeros(X.shape, np.int64), y, covar, weight, maxit, epsilon, dtype)
        self.F = X
        self.Fd = X.astype(dtype)
        self.proj = np.stack([(self.Fd * (self.w * self.Q[k])).sum(axis=1) for k in range(self.nb)], axis=1)
        # S_jj = sum (w x) x is a sum of non-negative terms: 0 exactly when every term is
        self.rsum = (((self.Fd * self.w) * self.Fd) != 0).any(axis=1).astype(np.int64)


class Backend(SR.Backend):
    """The restatement behind the interface of ``_DeviceScore`` with ``score_real_sets``."""

    def score(self, covar, weight, maxit, epsilon):
        self._fit = (covar, weight, maxit, epsilon)
        super().score(covar, weight, maxit, epsilon)

    def score_real_sets(self, rows, sets):
        self.Z = RealScore(rows, self.A.y, *self._fit, dtype=self.dtype).install(sets)
        self.n_sets = len(sets)
        return self.Z.proj.astype(np.float64), [S.astype(np.float64) for S in self.Z.S], self.Z.kept


# ---- the device comparisons' cases ----------------------------------------------------------------------------------------
# rows per case of assocscore_reference.CASES (kept samples 4 .. 2,097; covariates 0 / 0 / 1 / 5 / 12 / 6 / 3): 1, 15, 16, 17
# and 33 rows straddle the 16-row tiles of the Gram
ROWS = {"n5": 1, "n40": 15, "n255": 16, "n256": 17, "n257": 33, "n1000": 33, "n2100": 17}
SEEDS = {}                            # (offsets from SR.PERM_SEED of the first seed that meets the safety condition; the others 0)
_CACHE = {}


def seed_of(case):
    return SR.PERM_SEED + SEEDS.get(case, 0)


def real_rows(case):
    """X [m, n_kept]: random dosages in [0, 2], about half of them exact zeros; with m >= 4 the last row is all zero, the one
    before twice row 0, the one before that the constant 1.0."""
    m = ROWS[case]
    n = SR.analysis(case, "additive")[0].n
    rng = np.random.default_rng(1000 + m + n)
    X = rng.uniform(0.0, 2.0, (m, n)) * (rng.random((m, n)) < 0.5)
    if m >= 4:
        X[m - 1], X[m - 2], X[m - 3] = 0.0, 2.0 * X[0], 1.0
    return np.ascontiguousarray(X)


def real_sets(m):
    """Every row alone; the first d rows for d = 2, 15, 16, 17, 30 where there are that many; an empty set; with m >= 4 the
    aliased set (row 0, twice row 0, the constant, the zero row) and the last min(m, 30) rows."""
    sets = [[j] for j in range(m)]
    for d in (2, 15, 16, 17, 30):
        if d <= m:
            sets.append(list(range(d)))
    sets.append([])
    if m >= 4:
        sets.append([0, m - 2, m - 3, m - 1])
        sets.append(list(range(max(m - 30, 0), m)))
    return sets


def reference(case, dtype=np.float64, seed=None):
    """The RealScore of a case on ``real_rows`` and ``real_sets`` with SR.N_PERM[case] replicates (``perm_T``, ``max_stat``,
    ``count``), computed once per process and shared (callers do not modify it)."""
    seed = seed_of(case) if seed is None else seed
    key = (case, np.dtype(dtype).name, seed)
    if key not in _CACHE:
        A, covar, _, _ = SR.analysis(case, "additive")
        Z = RealScore(real_rows(case), A.y, covar, None, 25, 1e-8, dtype).install(real_sets(ROWS[case]))
        Z.seed = seed
        Z.perm_T = Z.stats(seed, 1, SR.N_PERM[case])
        Z.max_stat, Z.count = Z.max_and_count(Z.perm_T)
        _CACHE[key] = Z
    return _CACHE[key]


def tolerance_of(r, rl):
    """100 x the largest float64-versus-longdouble difference between two restatements of one case (SR.differences: section
    28's scales, with sum x^2 in place of the integer sums), at least 1e-12."""
    assert np.array_equal(r.flags, rl.flags) and np.array_equal(r.df, rl.df) and np.array_equal(r.kept, rl.kept)
    assert np.array_equal(r.count, rl.count)
    return max(100.0 * max(SR.differences(SR.numbers(r), SR.numbers(rl)).values()), 1e-12)


def tolerance(case):
    return tolerance_of(reference(case), reference(case, np.longdouble))


# ---- the end-to-end cohort ---------------------------------------------------------------------------------------------
E2E_SEED = 0x5EED0A550C1A7E01


def e2e_cohort():
    """The 200 x 3 synthetic cohort with a planted effect of its most frequent haplotype: (h1, h2, prob [3][200][2], alleles,
    y [200], covariates [200, 2])."""
    n, L, k, n_allele = 200, 3, 2, 8
    _, h1, h2, prob = R.ld_cohort(n, L, k, 6, n_allele, seed=21)
    key = "e2e"
    if key not in _CACHE:
        _CACHE[key] = dosages(h1, h2, prob)
    r = _CACHE[key]
    top = int(np.argmax(r["freq"]))
    rng = np.random.default_rng(77)
    cov = rng.standard_normal((n, 2))
    eta = -0.9 + 0.9 * np.nan_to_num(r["D"][top]) + 0.3 * cov[:, 0]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    return h1, h2, prob, n_allele, y, cov
