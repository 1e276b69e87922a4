"""CPU restatement of hlaAssocQuant for the tests: DESIGN.md section 25 items 1-9 in numpy, written from the definitions.

Dtype-generic: ``Quant`` takes ``dtype`` (``numpy.float64`` or ``numpy.longdouble``) and does all its arithmetic in it.
``perm_rows`` is the permutation generator (inside-out Fisher-Yates on Philox4x32-10 of tests/draws_reference.py), ``basis``
the orthonormalisation, ``Quant`` what the ``hibag_hip_assoc_quant_*`` entries return, ``Backend`` the same behind the
interface ``hibag_amd.assocquant`` drives, so that ``hlaAssocQuant`` itself runs on the restatement.  The samples, tests and
feature rows are those of tests/assoc_reference.py."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
from assoc_reference import allele_names, kept_columns       # noqa: F401  (the tests reach them through this module)
from draws_reference import philox4x32_10

MODELS = AR.MODELS
MAX_COVAR = 12
RANK_BIT = 2


class Collinear(ValueError):
    pass


def perm_rows(seed, perm0, n_perm, n):
    """int32 [n_perm, n]: row r is permutation perm0 + r (item 5); permutation 0 is the identity."""
    seed = int(seed)
    p = [int(perm0) + r for r in range(n_perm)]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    plo = np.array([v & 0xFFFFFFFF for v in p], np.uint64)
    phi = np.array([v >> 32 for v in p], np.uint64)
    rows = np.zeros((n_perm, n), np.int64)
    at = np.arange(n_perm)
    ident = np.array([v == 0 for v in p])
    w = None
    for i in range(n):
        if i & 3 == 0:
            counter = np.stack([np.full(n_perm, i >> 2, np.uint64), np.ones(n_perm, np.uint64), plo, phi], axis=-1)
            w = philox4x32_10(counter, key).astype(np.uint64)
        j = ((w[:, i & 3] * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
        j = np.where(ident, i, j)
        rows[at, i] = rows[at, j]
        rows[at, j] = i
    return rows.astype(np.int32)


def basis(covar, n, dtype=np.float64):
    """Q [1 + q, n]: the constant and the covariates [q, n], orthonormalised by modified Gram-Schmidt applied twice (item 2)."""
    Z = np.concatenate([np.ones((1, n)), np.asarray(covar, np.float64).reshape(-1, n)]).astype(dtype)
    Q = np.zeros_like(Z)
    for k in range(len(Z)):
        v = Z[k].copy()
        for _ in range(2):
            for j in range(k):
                c = (Q[j] * v).sum()
                v = v - c * Q[j]
        s = np.sqrt((v * v).sum())
        if not s > dtype(1e-9) * np.sqrt((Z[k] * Z[k]).sum()):
            raise Collinear("the covariates are collinear")
        Q[k] = v / s
    return Q


class Quant:
    """The trait y [n] with covariates [q, n] on the feature rows F [rows, n] of ``model``."""

    def __init__(self, F, model, y, covar=None, dtype=np.float64):
        self.dtype, self.model = dtype, model
        self.F = np.asarray(F, np.int64)
        rows, n = self.F.shape
        self.n = n
        self.T = rows // 2 if model == "genotype" else rows
        covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
        assert len(covar) <= MAX_COVAR
        self.nb = 1 + len(covar)
        d = 2 if model == "genotype" else 1
        if n - self.nb - d < 1:
            raise ValueError("no residual degree of freedom")
        y = np.asarray(y, np.float64)
        if not (np.isfinite(y).all() and np.isfinite(covar).all()):
            raise ValueError("not finite")
        self.Q = basis(covar, n, dtype)
        r = y.astype(dtype)
        for k in range(self.nb):
            c = (self.Q[k] * r).sum()
            r = r - c * self.Q[k]
        self.yt = r
        self.ybar = y.astype(dtype).sum() / dtype(n)
        self.yc = y.astype(dtype) - self.ybar
        # item 4: the class sums
        cls = self.F[0::2] + 2 * self.F[1::2] if model == "genotype" else self.F
        self.cnt = np.stack([(cls == k).sum(axis=1) for k in range(3)], axis=1).astype(np.int64)
        self.S1 = np.stack([np.where(cls == k, self.yc, dtype(0)).sum(axis=1) for k in range(3)], axis=1)
        self.S2 = np.stack([np.where(cls == k, self.yc * self.yc, dtype(0)).sum(axis=1) for k in range(3)], axis=1)
        # item 7: projections and the tests' constants
        self.Fd = self.F.astype(dtype)
        self.proj = self.Fd @ self.Q.T
        self.tests, self.flags = self._constants()
        self.g, rr, stat = self.run(np.arange(n)[None, :])
        self.rr, self.stat = rr[0], stat[:, 0]

    def _constants(self):
        """Per test None (not fitted) or (row_a, row_b, df, a11, a22, a12, det); row_b = -1 for one column, a11 = sxx."""
        dt, n, nb, P = self.dtype, self.n, self.nb, self.proj
        out, flags = [], np.full(self.T, RANK_BIT, np.int32)

        def sum_sq(row):
            return (P[row] * P[row]).sum()

        for t in range(self.T):
            c = self.cnt[t]
            out.append(None)
            if self.model == "genotype":
                if (c[1] == 0 and c[2] == 0) or c[0] == 0:
                    continue
                if c[1] > 0 and c[2] > 0:
                    xx1, xx2 = dt(c[1]), dt(c[2])
                    a11, a22 = xx1 - sum_sq(2 * t), xx2 - sum_sq(2 * t + 1)
                    a12 = -(P[2 * t] * P[2 * t + 1]).sum()
                    if not a11 > dt(1e-11) * xx1 or not a22 > dt(1e-11) * xx2:
                        continue
                    det = a11 * a22 - a12 * a12
                    if not det > dt(1e-11) * (a11 * a22):
                        continue
                    out[-1] = (2 * t, 2 * t + 1, dt(n - nb - 2), a11, a22, a12, det)
                    flags[t] = 0
                    continue
                row = 2 * t if c[1] > 0 else 2 * t + 1
                xx = dt(c[1] + c[2])
            else:
                if n in (c[0], c[1], c[2]):
                    continue
                row, xx = t, dt(c[1] + 4 * c[2])
            sxx = xx - sum_sq(row)
            if not sxx > dt(1e-11) * xx:
                continue
            out[-1] = (row, -1, dt(n - nb - 1), sxx, None, None, None)
            flags[t] = 0
        return out, flags

    def residuals(self, perms):
        """(r [P, n], rr [P]) of the permutation rows perms [P, n] (item 6)."""
        v = self.yt[np.asarray(perms, np.int64)]
        c = v @ self.Q.T
        r = v
        for k in range(self.nb):
            r = r - c[:, k:k + 1] * self.Q[k][None, :]
        return r, (r * r).sum(axis=1)

    def run(self, perms):
        """(g [rows, P], rr [P], T [n_test, P]) of the permutation rows (items 6 and 7)."""
        r, rr = self.residuals(perms)
        g = self.Fd @ r.T
        st = np.full((self.T, len(rr)), np.nan, self.dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            for t, c in enumerate(self.tests):
                if c is None:
                    continue
                row_a, row_b, df, a11, a22, a12, det = c
                if row_b < 0:
                    m = (g[row_a] * g[row_a]) / a11
                    d = 1
                else:
                    g1, g2 = g[row_a], g[row_b]
                    m = ((a22 * (g1 * g1) - ((2 * a12) * g1) * g2) + a11 * (g2 * g2)) / det
                    d = 2
                den = rr - m
                st[t] = np.where(den > 0, (m / d) / (den / df), np.nan)
        return g, rr, st

    def stats(self, seed, perm0, n_perm):
        """T [n_test, n_perm] of permutations perm0 .. perm0 + n_perm - 1."""
        return self.run(perm_rows(seed, perm0, n_perm, self.n))[2]

    def permute(self, seed, perm0, n_perm):
        """(max_stat [n_perm], count_point int64 [n_test]) as hibag_hip_assoc_quant_permute."""
        max_stat, count = AR.max_and_count(self.stats(seed, perm0, n_perm), self.stat)
        return max_stat.astype(np.float64), count

    def observed(self):
        f = np.float64
        return self.proj.astype(f), self.g[:, 0].astype(f), float(self.rr), self.stat.astype(f), self.flags


class Backend(AR.Backend):
    """The restatement behind the interface of hibag_amd.assocquant._DeviceQuant (``hlaAssocQuant(..., _backend=Backend)``)."""

    Z = None

    def quant(self, y, covar):
        try:
            self.Z = Quant(self.A.F, self.model, y, covar, self.dtype)
        except Collinear:
            raise ValueError("the covariates are collinear") from None

    def quant_classes(self):
        Z = self.Z
        return Z.cnt, Z.S1.astype(np.float64), Z.S2.astype(np.float64), float(Z.ybar)

    def quant_observed(self):
        return self.Z.observed()

    def quant_permute(self, seed, perm0, n_perm):
        return self.Z.permute(seed, perm0, n_perm)

    def quant_perm_rows(self, seed, perm0, n):
        return perm_rows(seed, perm0, n, self.n_kept)


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
# (samples, alleles, covariates, seed, samples with an unknown allele, with a partition whose level 1 is empty): the sample
# counts straddle the 128-sample padding of the handle and a 256-sample round of the device's walks, the allele counts the
# 16-row tiles of the Gram
CASES = {"n5": (5, 3, 0, 11, 1, False), "n40": (40, 6, 0, 12, 3, False), "n255": (255, 15, 1, 13, 3, False),
         "n256": (256, 16, 5, 14, 3, False), "n257": (257, 17, 12, 15, 3, False), "n1000": (1000, 65, 6, 16, 3, True)}
# The permutations compared per case: the first N_PERM[case] of a seed, and every shorter count listed in PERM_COUNTS as a
# prefix of them.  A permuted statistic EQUALS the observed one, up to rounding, whenever the permutation leaves a test's
# carriers in place (one homozygote in 37 samples: one permutation in 37), and the few samples of n5 and n40 have few
# permutations at all; which side of `>=` such a tie falls on is rounding, so the counts are compared under seeds without
# one (SEEDS: per case and model the first seed from PERM_SEED upwards that meets the safety condition ``min_gap > 1e-6``,
# found by tests/test_assocquant_host.py's rule and asserted there), and the small cohorts under fewer permutations.
N_PERM = {"n5": 1, "n40": 15, "n255": 200, "n256": 200, "n257": 200, "n1000": 200}
PERM_COUNTS = {"n5": (1,), "n40": (15,), "n255": (16, 200), "n256": (17, 200), "n257": (64, 200), "n1000": (65, 200)}
PERM_SEED = 0x9E3779B97F4A7C15       # a 64-bit seed
SEEDS = {("n40", "recessive"): 4}      # (offsets from PERM_SEED; the others 0)      # (offsets; the others 0)


def seed_of(case, model):
    return PERM_SEED + SEEDS.get((case, model), 0)


def min_gap(Z, seed, n_perm):
    """The safety condition's number: the smallest |T[t][p] - T_obs[t]| / T_obs[t] over the tests and permutations 1 .. n_perm."""
    st = Z.stats(seed, 1, n_perm)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.abs(st - Z.stat[:, None]) / Z.stat[:, None]
    return float(np.nanmin(gap)) if np.isfinite(gap).any() else np.inf


def cohort(n, n_allele, q, seed, n_na, partition=False):
    """(a1, a2, y float64, group_of or None, covar [q, n]): alleles drawn from frequencies ~ 0.93^k (sample k < n_allele
    carries allele k, so that every allele is in the data), y = 50 + effects of alleles 0 and 1 and of the covariates +
    noise, n_na of the other samples with an unknown allele."""
    rng = np.random.default_rng(seed)
    w = 0.93 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    a[:n_allele, 0] = np.arange(n_allele)
    covar = rng.standard_normal((q, n))
    gamma = rng.uniform(-1.0, 1.0, q)
    y = 50.0 + 1.5 * (a == 0).sum(axis=1) - 1.0 * (a == 1).any(axis=1) + gamma @ covar + 2.0 * rng.standard_normal(n)
    a[n_allele + rng.choice(n - n_allele, n_na, replace=False), rng.integers(0, 2, n_na)] = AR.NA_INTEGER
    g = AR.gap_partition(n_allele) if partition else None
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), y, g, covar


def hla_of(case):
    """The case's cohort as hlaAssocQuant takes it: (hla, y, groups or None, covar [n, q])."""
    n, n_allele, q, seed, n_na, partition = CASES[case]
    a1, a2, y, g, covar = cohort(n, n_allele, q, seed, n_na, partition)
    hla, _, groups = AR.hla_of(a1, a2, np.ones(n), n_allele, g)
    return hla, y, groups, covar.T


_CACHE = {}


def reference(case, model, dtype=np.float64):
    """The Quant of a case with its N_PERM[case] permuted runs under ``seed`` (``perm_g``, ``perm_rr``, ``perm_T``, ``max_stat``, ``count``),
    computed once per process and shared (callers do not modify it)."""
    key = (case, model, np.dtype(dtype).name)
    if key not in _CACHE:
        n, n_allele, q, seed, n_na, partition = CASES[case]
        a1, a2, y, g, covar = cohort(n, n_allele, q, seed, n_na, partition)
        y, covar = kept_columns(a1, a2, y, covar)
        A = AR.Analysis(a1, a2, np.zeros(n, np.int32), n_allele, g, model)
        Z = Quant(A.F, model, y, covar, dtype)
        Z.seed = seed_of(case, model)
        Z.perm_g, Z.perm_rr, Z.perm_T = Z.run(perm_rows(Z.seed, 1, N_PERM[case], Z.n))
        Z.max_stat, Z.count = AR.max_and_count(Z.perm_T, Z.stat)
        _CACHE[key] = Z
    return _CACHE[key]


def differences(got, want):
    """The largest differences between two sets of numbers of one case, each in units of the quantity's own scale (taken from
    ``want``): S1 in sqrt(cnt S2) and proj in sqrt(xx), g in sqrt(xx rr) -- the Cauchy-Schwarz bounds of those sums, which
    cancel --, S2 and rr relative, stat and max_stat in max(|T|, 1).  ``got`` / ``want``: dicts of cnt, S1, S2, proj, g, rr,
    stat, max_stat (arrays of any float dtype); ``xx`` [rows] is the feature rows' sum of squares."""
    ld = np.longdouble
    w = {k: np.asarray(v, ld) for k, v in want.items()}
    g = {k: np.asarray(v, ld) for k, v in got.items()}
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        full = w["cnt"] > 0
        out["S1"] = np.max((np.abs(g["S1"] - w["S1"]) / np.sqrt(w["cnt"] * w["S2"]))[full & (w["S2"] > 0)], initial=0)
        out["S2"] = np.max((np.abs(g["S2"] - w["S2"]) / w["S2"])[full & (w["S2"] > 0)], initial=0)
        some = w["xx"] > 0
        out["proj"] = np.max((np.abs(g["proj"] - w["proj"]) / np.sqrt(w["xx"])[:, None])[some], initial=0)
        out["g"] = np.max((np.abs(g["g"] - w["g"]) / np.sqrt(w["xx"] * w["rr"]))[some], initial=0)
        out["rr"] = np.abs(g["rr"] - w["rr"]) / w["rr"]
        for key in ("stat", "max_stat"):
            fin = np.isfinite(w[key])
            out[key] = np.max((np.abs(g[key] - w[key]) / np.fmax(np.abs(w[key]), 1))[fin], initial=0)
    return {k: float(v) for k, v in out.items()}


def numbers(Z):
    """The compared numbers of a reference() as ``differences`` takes them."""
    return dict(cnt=Z.cnt, S1=Z.S1, S2=Z.S2, proj=Z.proj, g=Z.g[:, 0], rr=Z.rr, stat=Z.stat, max_stat=Z.max_stat,
                xx=(Z.F * Z.F).sum(axis=1))


def tolerance(case, model):
    """100 x the largest float64-versus-longdouble difference of the restatement over the case (``differences``), at least
    1e-12."""
    r, rl = reference(case, model), reference(case, model, np.longdouble)
    assert np.array_equal(r.flags, rl.flags) and np.array_equal(r.count, rl.count)
    return max(100.0 * max(differences(numbers(r), numbers(rl)).values()), 1e-12)
