"""CPU restatement of hlaAssocScore for the tests: DESIGN.md section 28 items 1-9 in numpy, written from the definitions.

Dtype-generic: ``Score`` takes ``dtype`` (``numpy.float64`` or ``numpy.longdouble``) and does all its arithmetic in it.
``signs`` is the sign generator (Philox4x32-10 of tests/draws_reference.py), ``weighted_basis`` the orthonormalisation under
the model's weights, ``Score`` what the ``hibag_hip_assoc_score_*`` entries return, ``Backend`` the same behind the interface
``hibag_amd.assocscore`` drives, so that ``hlaAssocScore`` itself runs on the restatement.  The base fit is that of
tests/assocglm_reference.py; the samples, tests and feature rows are those of tests/assoc_reference.py."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
import assocglm_reference as G
import assocomni_reference as OM
from assoc_reference import allele_names, kept_columns       # noqa: F401  (the tests reach them through this module)
from draws_reference import philox4x32_10

MODELS = AR.MODELS
MAX_COVAR, MAX_ROWS = 12, 30
MAXIT_BIT, RANK_BIT, ALIASED_BIT = 1, 2, 8


class Collinear(ValueError):
    pass


def signs(seed, p0, n_perm, n):
    """int8 [n_perm, n]: row r is replicate p0 + r (item 5): bit p & 127 of Philox4x32-10(counter (i, 2, (p >> 7) lo,
    (p >> 7) hi), key (seed lo, seed hi)) set means -1; replicate 0 is all +1."""
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    out = np.ones((n_perm, n), np.int8)
    i = np.arange(n, dtype=np.uint64)
    words, have = None, None
    for r in range(n_perm):
        p = int(p0) + r
        if p == 0:
            continue
        blk = p >> 7
        if blk != have:
            counter = np.stack([i, np.full(n, 2, np.uint64), np.full(n, blk & 0xFFFFFFFF, np.uint64), np.full(n, blk >> 32, np.uint64)],
                               axis=-1)
            words, have = philox4x32_10(counter, key).astype(np.uint64), blk
        at = p & 127
        out[r] = np.where((words[:, at >> 5] >> np.uint64(at & 31)) & np.uint64(1), -1, 1)
    return out


def weighted_basis(Z, w, dtype=np.float64):
    """Q [len(Z), n] with Q' W Q = I: the rows of Z orthonormalised by modified Gram-Schmidt applied twice under the inner
    product sum_i (w_i a_i) b_i (item 3)."""
    Z = np.asarray(Z).astype(dtype)
    Q = np.zeros_like(Z)
    for k in range(len(Z)):
        v = Z[k].copy()
        for _ in range(2):
            for j in range(k):
                c = ((w * Q[j]) * v).sum()
                v = v - c * Q[j]
        s = np.sqrt(((w * v) * v).sum())
        if not s > dtype(1e-9) * np.sqrt(((w * Z[k]) * Z[k]).sum()):
            raise Collinear("the covariates are collinear")
        Q[k] = v / s
    return Q


class Score:
    """The case / control trait y [n] with covariates [q, n] and prior weights on the feature rows F [rows, n]."""

    def __init__(self, F, y, covar=None, weight=None, maxit=25, epsilon=1e-8, dtype=np.float64):
        self.dtype = dt = dtype
        self.F = np.asarray(F, np.int64)
        rows, n = self.F.shape
        self.n = n
        covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
        assert len(covar) <= MAX_COVAR
        self.nb = 1 + len(covar)
        wt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
        Z = np.concatenate([np.ones((1, n)), covar])
        # item 2: the base fit, then eta, mu, v, w, e from its coefficients
        self.base = G.fit(Z.T, y, wt, maxit, epsilon, dt)
        if self.base["flags"] & RANK_BIT:
            raise Collinear("the base model is rank-deficient")
        beta = np.asarray(self.base["coef"], dt)
        Zd = Z.astype(dt)
        eta = np.full(n, beta[0], dt)
        for k in range(1, self.nb):
            eta = eta + Zd[k] * beta[k]
        _, mu = G._mean(eta, dt)
        self.mu = mu
        self.w = wt.astype(dt) * (mu * (1 - mu))
        self.e = wt.astype(dt) * (np.asarray(y).astype(dt) - mu)
        self.Q = weighted_basis(Z, self.w, dt)
        self.Fd = self.F.astype(dt)
        self.rsum = self.F.sum(axis=1)
        self.proj = np.stack([(self.Fd * (self.w * self.Q[k])).sum(axis=1) for k in range(self.nb)], axis=1)
        self.ratios = []

    def install(self, sets):
        """Item 4 for the sets of feature rows: S, V, the factor with aliased columns dropped, kept masks, df and flags; then
        the observed run (replicate 0)."""
        dt = self.dtype
        self.sets = [list(s) for s in sets]
        self.S, self.kept_rows, self.L, self.kept = [], [], [], np.zeros(len(sets), np.int32)
        self.df, self.flags = np.zeros(len(sets), np.int32), np.zeros(len(sets), np.int32)
        failed = bool(self.base["flags"] & MAXIT_BIT)
        for t, rows in enumerate(self.sets):
            assert len(rows) <= MAX_ROWS and len(set(rows)) == len(rows)
            X = self.Fd[rows] if rows else np.zeros((0, self.n), dt)
            S = (X * self.w) @ X.T
            P = self.proj[rows] if rows else np.zeros((0, self.nb), dt)
            V = S.copy()
            for a in range(len(rows)):
                for b in range(len(rows)):
                    pp = dt(0)
                    for k in range(self.nb):
                        pp = pp + P[a, k] * P[b, k]
                    V[a, b] = S[a, b] - pp
            keep, Lr = [], []
            for j in range(len(rows)):
                if self.rsum[rows[j]] == 0:
                    continue
                row = []
                for i, m in enumerate(keep):
                    v = V[j, m]
                    for c in range(i):
                        v = v - row[c] * Lr[i][c]
                    row.append(v / Lr[i][i])
                d = V[j, j]
                for v in row:
                    d = d - v * v
                self.ratios.append(float(d / S[j, j]))
                if not d > dt(1e-11) * S[j, j]:
                    continue
                Lr.append(row + [np.sqrt(d)])
                keep.append(j)
            self.S.append(S)
            self.kept[t] = sum(1 << j for j in keep)
            fl = RANK_BIT if not keep else ALIASED_BIT if len(keep) < len(rows) else 0
            if failed:
                fl, keep, Lr = fl | MAXIT_BIT, [], []
            self.flags[t], self.df[t] = fl, len(keep)
            self.kept_rows.append([rows[j] for j in keep])
            self.L.append(Lr)
        self.dfs = sorted(set(self.df[self.df > 0].tolist()))
        self.g, T = self.run(np.ones((1, self.n), np.int8))
        self.g, self.stat = self.g[:, 0], T[:, 0]
        return self

    def residuals(self, sg):
        """r [P, n] of the sign rows sg [P, n] (item 6)."""
        v = self.e[None, :] * np.asarray(sg).astype(self.dtype)
        c = v @ self.Q.T
        t = np.zeros_like(v)
        for k in range(self.nb):
            t = t + c[:, k:k + 1] * self.Q[k][None, :]
        return v - self.w[None, :] * t

    def run(self, sg):
        """(g [rows, P], T [n_sets, P]) of the sign rows (items 6 and 7)."""
        r = self.residuals(sg)
        g = self.Fd @ r.T
        T = np.full((len(self.sets), len(r)), np.nan, self.dtype)
        for s, (rows, L) in enumerate(zip(self.kept_rows, self.L)):
            if not rows:
                continue
            ts, tot = [], None
            for a, row in enumerate(rows):
                v = g[row]
                for b in range(a):
                    v = v - L[a][b] * ts[b]
                ta = v / L[a][a]
                ts.append(ta)
                tot = ta * ta if tot is None else tot + ta * ta
            T[s] = tot
        self.last_r = r
        return g, T

    def stats(self, seed, p0, n_perm):
        return self.run(signs(seed, p0, n_perm, self.n))[1]

    def max_and_count(self, T):
        """(max_stat [P, n_df], count_point int64 [n_sets]) of the statistics T [n_sets, P] (item 8)."""
        cols = []
        for d in self.dfs:
            best, _ = AR.max_and_count(T[self.df == d], self.stat[self.df == d])
            cols.append(best)
        max_stat = np.stack(cols, axis=1) if cols else np.zeros((T.shape[1], 0))
        with np.errstate(invalid="ignore"):
            count = (T >= self.stat[:, None]).sum(axis=1).astype(np.int64)
        return max_stat.astype(np.float64), count

    def resample(self, seed, p0, n_perm):
        return self.max_and_count(self.stats(seed, p0, n_perm))


class Backend(OM.Backend):
    """The restatement behind the interface of hibag_amd.assocscore._DeviceScore (``hlaAssocScore(..., _backend=Backend)``)."""

    Z = None
    n_sets = 0

    @property
    def n_rows(self):
        return len(self.A.F)

    def score(self, covar, weight, maxit, epsilon):
        try:
            self.Z = Score(self.A.F, self.A.y, covar, weight, maxit, epsilon, self.dtype)
        except Collinear:
            raise ValueError("the covariates are collinear (the base model is rank-deficient)") from None

    def score_base(self):
        b, q = self.Z.base, self.Z.nb - 1
        coef, se = np.full(G.SLOTS, np.nan), np.full(G.SLOTS, np.nan)
        used = [0] + list(range(G.COV0, G.COV0 + q))
        coef[used], se[used] = np.asarray(b["coef"], np.float64), np.asarray(b["se"], np.float64)
        return coef, se, float(b["deviance"]), int(b["iterations"]), int(b["flags"])

    def score_sets(self, sets):
        Z = self.Z.install(sets)
        self.n_sets = len(sets)
        return Z.proj.astype(np.float64), [S.astype(np.float64) for S in Z.S], Z.kept

    def score_observed(self):
        Z = self.Z
        return Z.g.astype(np.float64), Z.stat.astype(np.float64), Z.df, Z.flags

    def score_resample(self, seed, p0, n_perm):
        return self.Z.resample(seed, p0, n_perm)

    def score_signs(self, seed, p0, n):
        return signs(seed, p0, n, self.n_kept)


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
# (samples, alleles, covariates, seed, samples with an unknown allele, with a partition whose level 1 is empty): the sample
# counts straddle the 128-sample padding of the handle, the 256-sample chunks and 1,024-sample segments of the residual
# kernels and a 256-sample round of the device's walks, the allele counts the 16-row tiles of the Gram
CASES = {"n5": (5, 3, 0, 31, 1, False), "n40": (40, 6, 0, 32, 3, False), "n255": (255, 15, 1, 33, 3, False),
         "n256": (256, 16, 5, 34, 3, False), "n257": (257, 17, 12, 35, 3, False), "n1000": (1000, 65, 6, 36, 3, True),
         "n2100": (2100, 20, 3, 37, 3, True)}      # (2,097 kept samples: three segments of the residual kernels' walk, the last of 49)
# The replicates compared per case: the first N_PERM[case] of a seed, and every count listed in PERM_COUNTS as a prefix of
# them.  Four kept samples (n5) have sixteen sign patterns, two of which give the observed statistic again; which side of
# `>=` such a tie falls on is rounding, so the counts are compared under seeds without one (``seed_of``: per case and model
# the first seed from PERM_SEED upwards that meets the safety condition, found by tests/test_assocscore_host.py's rule and
# asserted there), and n5 under one replicate.
N_PERM = {"n5": 1, "n40": 17, "n255": 200, "n256": 200, "n257": 200, "n1000": 200, "n2100": 200}
PERM_COUNTS = {"n5": (1,), "n40": (15, 16, 17), "n255": (1, 127, 200), "n256": (16, 128, 200), "n257": (17, 129, 200),
               "n1000": (15, 128, 200), "n2100": (129, 200)}
PERM_SEED = 0xD1B54A32D192ED03       # a 64-bit seed
SEEDS = {}                            # (offsets from PERM_SEED; the others 0)
SAFETY = 1e-6


def seed_of(case, model):
    return PERM_SEED + SEEDS.get((case, model), 0)


def cohort(n, n_allele, q, seed, n_na, partition=False):
    """(a1, a2, y int32, group_of or None, covar [q, n], prob [n]): alleles drawn from frequencies ~ 0.93^k (sample k < n_allele
    carries allele k, so that every allele is in the data, and homozygotes occur), y from a logistic model with the effects of
    alleles 0 and 1 and of the covariates (sample 0 a case, sample 1 a control), n_na of the other samples with an unknown
    allele, ``prob`` uniform on (0.3, 1)."""
    rng = np.random.default_rng(seed)
    w = 0.93 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    a[:n_allele, 0] = np.arange(n_allele)
    covar = rng.standard_normal((q, n))
    gamma = rng.uniform(-0.5, 0.5, q) / np.sqrt(max(q, 1))
    eta = -0.3 + 0.8 * (a == 0).any(axis=1) - 0.7 * (a == 1).any(axis=1) + gamma @ covar
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    y[0], y[1] = 1, 0
    a[n_allele + rng.choice(n - n_allele, n_na, replace=False), rng.integers(0, 2, n_na)] = AR.NA_INTEGER
    prob = rng.uniform(0.3, 1.0, n)
    g = AR.gap_partition(n_allele) if partition else None
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), y, g, covar, prob


def hla_of(case):
    """The case's cohort as hlaAssocScore takes it: (hla with ``prob``, y, groups or None, covar [n, q])."""
    n, n_allele, q, seed, n_na, partition = CASES[case]
    a1, a2, y, g, covar, prob = cohort(n, n_allele, q, seed, n_na, partition)
    hla, _, groups = AR.hla_of(a1, a2, prob, n_allele, g)
    return hla, y, groups, covar.T


def single_sets(model, rsum, n):
    """Every test's set by section 23 item 6's rules (hibag_amd.assocscore._single_sets, restated)."""
    if model == "genotype":
        out = []
        for t in range(len(rsum) // 2):
            het, hom = int(rsum[2 * t]), int(rsum[2 * t + 1])
            out.append([] if (het == 0 and hom == 0) or het + hom == n else [2 * t + j for j, r in enumerate((het, hom)) if r > 0])
        return out
    top = (2 if model == "additive" else 1) * n
    return [[] if int(r) in (0, top) else [t] for t, r in enumerate(rsum)]


def run_sets(case, model, A):
    """The sets of a device run: every test's own set; sets of the first d feature rows after row 0 for d = 1, 2, 15, 16, 17
    and 30 where the handle has the rows; an empty set; all allele rows at once where they fit (``additive``: they add up to 2,
    so the last is aliased exactly); and, with the gap partition, a row nobody carries beside two that are carried."""
    sets = single_sets(model, A.rsum, A.n)
    rows = len(A.F)
    for d in (1, 2, 15, 16, 17, 30):
        if 1 + d <= rows:
            sets.append(list(range(1, 1 + d)))
    sets.append([])
    n_allele = CASES[case][1]
    per = 2 if model == "genotype" else 1
    if per * n_allele <= MAX_ROWS:
        sets.append(list(range(per * n_allele)))
    if CASES[case][5]:
        gap = [per * (n_allele + lv) for lv in range(3)]
        assert A.rsum[gap[1]] == 0
        sets.append(gap)
    return sets


_CACHE = {}


def analysis(case, model):
    key = (case, model)
    if key not in _CACHE:
        n, n_allele, q, seed, n_na, partition = CASES[case]
        a1, a2, y, g, covar, prob = cohort(n, n_allele, q, seed, n_na, partition)
        covar, prob = kept_columns(a1, a2, covar, prob)
        _CACHE[key] = (AR.Analysis(a1, a2, y, n_allele, g, model), covar, prob, (a1, a2, y, n_allele, g))
    return _CACHE[key]


def reference(case, model, dtype=np.float64, seed=None):
    """The Score of a case on ``run_sets`` with its N_PERM[case] replicates under ``seed`` (``perm_T``, ``max_stat``, ``count``; the
    case's own seed by default), computed once per process and shared (callers do not modify it)."""
    seed = seed_of(case, model) if seed is None else seed
    key = (case, model, np.dtype(dtype).name, seed)
    if key not in _CACHE:
        A, covar, _, _ = analysis(case, model)
        Z = Score(A.F, A.y, covar, None, 25, 1e-8, dtype).install(run_sets(case, model, A))
        Z.seed = seed
        Z.perm_T = Z.stats(seed, 1, N_PERM[case])
        Z.perm_rr = (Z.last_r * Z.last_r).sum(axis=1)
        Z.max_stat, Z.count = Z.max_and_count(Z.perm_T)
        _CACHE[key] = Z
    return _CACHE[key]


def min_p(max_stat, dfs):
    from hibag_amd.assocscore import _min_p
    return _min_p(np.asarray(max_stat, np.float64), dfs)


def score_p(Z):
    from hibag_amd.assoc import chisq_sf
    return np.array([chisq_sf(float(s), int(d)) if d > 0 else np.nan for s, d in zip(Z.stat, Z.df)])


def min_gap(Z, T):
    """The safety condition's numbers over the statistics T [n_sets, P]: the smallest |T[t][p] - T[t][0]| / T[t][0], and the
    smallest |min_p[p] - score_p[t]| / score_p[t]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.abs(T - Z.stat[:, None]) / Z.stat[:, None]
        g1 = float(np.nanmin(gap)) if np.isfinite(gap).any() else np.inf
        mp = min_p(Z.max_and_count(T)[0], Z.dfs)
        sp = score_p(Z)
        gp = np.abs(mp[None, :] - sp[:, None]) / sp[:, None]
        g2 = float(np.nanmin(gp)) if np.isfinite(gp).any() else np.inf
    return g1, g2


def differences(got, want):
    """The largest differences between two sets of numbers of one case, each in units of the quantity's own scale (taken from
    ``want``): proj in sqrt(S_rr) and S in sqrt(S_aa S_bb) -- the Cauchy-Schwarz bounds of those sums under the weights --,
    g in sqrt(xx rr), stat and max_stat in max(|T|, 1).  ``got`` / ``want``: dicts of proj, S (a list per set), g, stat,
    max_stat, with ``srr`` [rows] = sum w F^2, ``xx`` [rows] = sum F^2 and ``rr`` = sum r^2 of the observed run."""
    ld = np.longdouble
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        srr, xx, rr = np.asarray(want["srr"], ld), np.asarray(want["xx"], ld), ld(want["rr"])
        some = srr > 0
        out["proj"] = np.max((np.abs(np.asarray(got["proj"], ld) - np.asarray(want["proj"], ld)) / np.sqrt(srr)[:, None])[some], initial=0)
        out["g"] = np.max((np.abs(np.asarray(got["g"], ld) - np.asarray(want["g"], ld)) / np.sqrt(xx * rr))[some], initial=0)
        worst = ld(0)
        for a, b in zip(got["S"], want["S"]):
            a, b = np.asarray(a, ld), np.asarray(b, ld)
            d = np.sqrt(np.outer(np.diag(b), np.diag(b)))
            if a.size and (d > 0).any():
                worst = max(worst, np.max((np.abs(a - b) / d)[d > 0]))
        out["S"] = worst
        for key in ("stat", "max_stat"):
            w, g = np.asarray(want[key], ld), np.asarray(got[key], ld)
            fin = np.isfinite(w)
            out[key] = np.max((np.abs(g - w) / np.fmax(np.abs(w), 1))[fin], initial=0)
    return {k: float(v) for k, v in out.items()}


def numbers(Z):
    """The compared numbers of a reference() as ``differences`` takes them."""
    r0 = Z.residuals(np.ones((1, Z.n), np.int8))[0]
    return dict(proj=Z.proj, S=Z.S, g=Z.g, stat=Z.stat, max_stat=Z.max_stat, srr=(Z.Fd * Z.Fd * Z.w).sum(axis=1),
                xx=(Z.F * Z.F).sum(axis=1), rr=(r0 * r0).sum())


def tolerance(case, model):
    """100 x the largest float64-versus-longdouble difference of the restatement over the case (``differences``), at least
    1e-12."""
    r, rl = reference(case, model), reference(case, model, np.longdouble)
    assert np.array_equal(r.flags, rl.flags) and np.array_equal(r.df, rl.df) and np.array_equal(r.kept, rl.kept)
    assert np.array_equal(r.count, rl.count)
    return max(100.0 * max(differences(numbers(r), numbers(rl)).values()), 1e-12)
