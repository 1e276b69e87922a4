"""CPU restatement of hlaAssocOmnibus for the tests: DESIGN.md section 26 in numpy, written from the definitions.

``fit`` is one IRLS fit of section 23 items 3-5 on the design ``[1 | rows | covariates]`` with the drop rule of section 26
item 2 (factorisation order: intercept, covariates, rows; a column whose pivot is <= 1e-11 A_jj leaves the fit for good);
``glm_sets`` is what ``hibag_hip_assoc_glm_sets`` returns (the fits of all sets and the base model, by slot, with the set rules
of item 3); ``design_sets`` the set of a partition (item 4: carried levels, reference level); ``chisq_sf`` the chi-square tail;
``Backend`` all of it behind the interface ``hibag_amd.assocomni`` drives.  Dtype-generic like tests/assocglm_reference.py,
whose triangular solves it uses; the samples, tests and feature rows are those of tests/assoc_reference.py."""

from __future__ import annotations

import math

import numpy as np

import assoc_reference as AR
import assocglm_reference as G

MODELS = AR.MODELS
SLOTS, MAX_COLUMNS = 32, 30
MAXIT_BIT, RANK_BIT, BOUNDARY_BIT, ALIASED_BIT, TOO_WIDE_BIT = 1, 2, 4, 8, 16


def cholesky_drop(A, dtype, ratios):
    """Column-order Cholesky of A (column 0 the intercept) that drops a column whose pivot is <= 1e-11 A_jj: (kept, L) with L
    the factor of A[kept][:, kept], or None where the intercept fails.  Every pivot ratio d_j / A_jj goes to ``ratios``."""
    kept, rows = [], []
    for j in range(len(A)):
        row = []
        for i, m in enumerate(kept):
            v = A[j, m]
            for t in range(i):
                v = v - row[t] * rows[i][t]
            row.append(v / rows[i][i])
        d = A[j, j]
        for v in row:
            d = d - v * v
        if A[j, j] > 0:
            ratios.append(float(d / A[j, j]))
        if not d > dtype(1e-11) * A[j, j]:
            if j == 0:
                return None
            continue
        rows.append(row + [np.sqrt(d)])
        kept.append(j)
    L = np.zeros((len(kept), len(kept)), dtype)
    for i, row in enumerate(rows):
        L[i, :i + 1] = row
    return kept, L


def fit(X, n_h, y, wt, maxit=25, epsilon=1e-8, dtype=np.float64):
    """One fit on X = [1 | n_h rows | covariates]: dict coef, se [p] in the order of X (NaN for a dropped column), deviance,
    iterations, flags, df_h (the rows still in the last solve), crit (every iteration's), ratios (every pivot ratio)."""
    X = np.asarray(X, dtype)
    y = np.asarray(y, dtype)
    wt = np.asarray(wt, dtype)
    eps = dtype(2.0) ** -52
    p = X.shape[1]
    active = [0] + list(range(1 + n_h, p)) + list(range(1, 1 + n_h))       # the factorisation order
    nan = np.full(p, np.nan)
    mu = (wt * y + dtype(0.5)) / (wt + 1)
    eta = np.log(mu / (1 - mu))
    devold = G._deviance(mu, y, wt)
    crits, ratios = [], []
    flags = 0
    for k in range(1, maxit + 1):
        t, mu = G._mean(eta, dtype)
        g = np.where(np.abs(eta) > 30, eps, t / ((1 + t) * (1 + t)))
        v = mu * (1 - mu)
        z = eta + (y - mu) / g
        W = wt * (g * g) / v
        Xa = X[:, active]
        A = Xa.T @ (Xa * W[:, None])
        b = Xa.T @ (W * z)
        res = cholesky_drop(A, dtype, ratios)
        if res is None:
            return dict(coef=nan, se=nan, deviance=np.nan, iterations=k, flags=flags | RANK_BIT, df_h=0, crit=crits, ratios=ratios)
        kept, L = res
        if len(kept) < len(active):
            flags |= ALIASED_BIT
        active = [active[j] for j in kept]
        beta = G.solve(L, b[kept], dtype)
        eta = X[:, active] @ beta
        _, mu = G._mean(eta, dtype)
        dev = G._deviance(mu, y, wt)
        crit = abs(dev - devold) / (abs(dev) + dtype(0.1))
        crits.append(float(crit))
        if crit < epsilon:
            break
        devold = dev
    else:
        flags |= MAXIT_BIT
    if ((mu < 10 * eps) | (mu > 1 - 10 * eps)).any():
        flags |= BOUNDARY_BIT
    coef, se = np.full(p, np.nan, dtype), np.full(p, np.nan, dtype)
    coef[active], se[active] = beta, np.sqrt(G.inverse_diagonal(L, dtype))
    return dict(coef=coef, se=se, deviance=dev, iterations=k, flags=flags, df_h=sum(1 for j in active if 1 <= j <= n_h),
                crit=crits, ratios=ratios)


def glm_sets(F, sets, covar, weight, y, maxit=25, epsilon=1e-8, dtype=np.float64):
    """What hibag_hip_assoc_glm_sets returns from the feature rows F [rows, n] and the sets (lists of row indices): dict of
    coef, se [n_sets + 1, 32] by slot (float64), deviance, iterations, flags, df_h [n_sets + 1], and crit / ratios, lists per
    fit; the last fit is the base model."""
    n = F.shape[1]
    covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
    q = len(covar)
    assert q <= MAX_COLUMNS - 1
    wt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    rsum = F.sum(axis=1)
    for s in sets:
        assert len(set(s)) == len(s) and all(0 <= r < len(F) for r in s)
    fitted = [len(s) <= MAX_COLUMNS - q and any(rsum[r] > 0 for r in s) for s in sets]
    H = max([len(s) for s, ok in zip(sets, fitted) if ok], default=0)
    n_fit = len(sets) + 1
    out = dict(coef=np.full((n_fit, SLOTS), np.nan), se=np.full((n_fit, SLOTS), np.nan), deviance=np.full(n_fit, np.nan),
               iterations=np.zeros(n_fit, np.int32), flags=np.zeros(n_fit, np.int32), df_h=np.zeros(n_fit, np.int32),
               crit=[[] for _ in range(n_fit)], ratios=[[] for _ in range(n_fit)], H=H)
    for f, s in enumerate(list(sets) + [[]]):
        if f < len(sets) and not fitted[f]:
            out["flags"][f] = RANK_BIT | (TOO_WIDE_BIT if len(s) > MAX_COLUMNS - q else 0)
            continue
        carried = [j for j, r in enumerate(s) if rsum[r] > 0]                # a row nobody carries is left out before the fit
        slots = [0] + [1 + j for j in carried] + list(range(1 + H, 1 + H + q))
        cols = [np.ones(n)] + [F[s[j]].astype(np.float64) for j in carried] + list(covar)
        res = fit(np.stack(cols, axis=1), len(carried), y, wt, maxit, epsilon, dtype)
        out["coef"][f, slots] = np.asarray(res["coef"], np.float64)
        out["se"][f, slots] = np.asarray(res["se"], np.float64)
        out["deviance"][f] = float(res["deviance"])
        out["iterations"][f], out["df_h"][f] = res["iterations"], res["df_h"]
        out["flags"][f] = res["flags"] | (ALIASED_BIT if len(carried) < len(s) else 0)
        out["crit"][f], out["ratios"][f] = res["crit"], res["ratios"]
    return out


def design_sets(part_rows, rsum):
    """Per partition (its set as level indices, its reference level or -1, the number of carried levels), from the feature
    row of every level (-1: unknown to the device) and the row sums: carried = known with a positive sum; the reference is
    the carried level with the largest sum, the lowest index on a tie; fewer than two carried levels: no set."""
    sets, ref, n_carried = [], [], []
    for rows in part_rows:
        carried = [lv for lv, r in enumerate(rows) if r >= 0 and rsum[r] > 0]
        n_carried.append(len(carried))
        if len(carried) < 2:
            sets.append([])
            ref.append(-1)
            continue
        top = max(int(rsum[rows[lv]]) for lv in carried)
        r0 = min(lv for lv in carried if int(rsum[rows[lv]]) == top)
        ref.append(r0)
        sets.append([lv for lv in carried if lv != r0])
    return sets, ref, n_carried


def chisq_sf(x, df):
    """The chi-square upper tail for an integer df >= 1 from the closed forms, term by term (math.fsum of the series)."""
    if math.isnan(x) or df < 1:
        return math.nan
    h = max(x, 0.0) / 2.0
    if df % 2 == 0:
        return math.exp(-h) * math.fsum(h ** k / math.factorial(k) for k in range(df // 2))
    series = math.fsum(h ** (k - 0.5) / math.gamma(k + 0.5) for k in range(1, (df - 1) // 2 + 1))
    return math.erfc(math.sqrt(h)) + math.exp(-h) * series


class Backend(G.Backend):
    """The restatement behind the interface of hibag_amd.assocomni._DeviceOmni (``hlaAssocOmnibus(..., _backend=Backend)``)."""

    LOG = []          # (crit, ratios) of every call, for the safety conditions of tests/test_assocomni_host.py

    def row_sums(self):
        return self.A.rsum.astype(np.int32)

    def glm_sets(self, sets, covar, weight, maxit, epsilon):
        r = glm_sets(self.A.F, [list(s) for s in sets], covar, weight, self.A.y, maxit, epsilon, self.dtype)
        Backend.LOG.append((r["crit"], r["ratios"]))
        return r["coef"], r["se"], r["deviance"], r["iterations"], r["flags"], r["df_h"]


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
# (samples, alleles, seed, extra partitions).  Three samples of every cohort have an unknown allele, so the KEPT samples, which
# the cases are named for, number 40 / 255 / 256 / 257 / 1000: they straddle the handle's padding to 128 (256 kept samples
# have no padding sample and a full last step; 257 have one real sample before 127 padding samples) and a 256-sample
# boundary of the device's walk (eight waves of four samples per step).  Every cohort has 29 covariates; a run takes the
# first q.
CASES = {"n40": (43, 6, 21, False), "n255": (258, 10, 22, False), "n256": (259, 10, 23, False), "n257": (260, 12, 24, False),
         "n1000": (1003, 24, 25, True)}
KEPT = {"n40": 40, "n255": 255, "n256": 256, "n257": 257, "n1000": 1000}
CASE_Q = {"n40": 0, "n255": 1, "n256": 5, "n257": 12, "n1000": 6}
Q_MAX = 29


def partitions(n_allele, extra):
    """(names, levels, group_of): partitions of 2, 3, 5 and 8 levels (p2 names one level more than any allele has: unknown to
    the device); with ``extra`` also ``gap`` (its level 1 is empty), ``p3b`` (the levels of p3 under other numbers) and
    ``all`` (every allele a level of its own)."""
    a = np.arange(n_allele)
    names, rows = ["p2", "p3", "p5", "p8"], [a % 2, a % 3, a % 5, a % 8]
    if extra:
        names += ["gap", "p3b", "all"]
        rows += [np.where(a % 3 == 0, 0, 2 + a % 2), (a % 3 + 1) % 3, a]
    g = np.stack(rows).astype(np.int32)
    levels = [[f"{nm}.{k}" for k in range(int(r.max()) + 1)] for nm, r in zip(names, g)]
    levels[0].append("p2.beyond")
    return names, levels, g


def cohort(n, n_allele, seed, extra=False):
    """(a1, a2, y, group_of, covar [29, n], prob [n]): alleles drawn from frequencies ~ 0.9^k, y from a logistic model with
    the effects of the levels 1 and 2 of p3 (per allele copy) and of the first covariates, three samples with an unknown
    allele, ``prob`` uniform on (0.3, 1) with two zeros."""
    rng = np.random.default_rng(seed)
    w = 0.9 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    covar = rng.standard_normal((Q_MAX, n))
    gamma = np.zeros(Q_MAX)
    gamma[:6] = rng.uniform(-0.5, 0.5, 6) / np.sqrt(6)
    eta = -0.3 + 0.8 * (a % 3 == 1).sum(axis=1) - 0.7 * (a % 3 == 2).sum(axis=1) + gamma @ covar
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    a[rng.choice(n, 3, replace=False), rng.integers(0, 2, 3)] = AR.NA_INTEGER
    prob = rng.uniform(0.3, 1.0, n)
    prob[rng.choice(n, 2, replace=False)] = 0.0
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), y, partitions(n_allele, extra)[2], covar, prob


_ANALYSIS = {}


def analysis(case, model):
    """(AR.Analysis, covar [29, n_kept], prob [n_kept], part_rows) of a case, computed once per process."""
    key = (case, model)
    if key not in _ANALYSIS:
        n, n_allele, seed, extra = CASES[case]
        a1, a2, y, g, covar, prob = cohort(n, n_allele, seed, extra)
        covar, prob = AR.kept_columns(a1, a2, covar, prob)
        A = AR.Analysis(a1, a2, y, n_allele, g, model)
        assert A.n == KEPT[case]
        part_rows, at = [], n_allele
        for row in g:
            k = int(row.max()) + 1
            part_rows.append(list(range(at, at + k)))
            at += k
        _ANALYSIS[key] = (A, covar, prob, part_rows)
    return _ANALYSIS[key]


def run_sets(case, model, q):
    """The sets of a device run: every partition's omnibus set; sets of allele rows 1 .. d (allele 0, the most frequent, is
    the reference) with 1 + d + q = 15, 16, 17 and 31 where the cohort has the alleles; an empty set; a row nobody carries
    beside two that are carried (n1000: level 1 of ``gap``); all alleles at once (``additive``: they add up to 2, so the
    last is aliased exactly); and, where the handle has the rows, one set too wide for the design."""
    A, _, _, part_rows = analysis(case, model)
    n_allele = CASES[case][1]
    sets = [[rows[lv] for lv in s] for rows, s in zip(part_rows, design_sets(part_rows, A.rsum)[0])]
    for total in (15, 16, 17, 31):
        d = total - 1 - q
        if 1 <= d <= n_allele - 1:
            sets.append(list(range(1, 1 + d)))
    sets.append([])
    if CASES[case][3]:
        gap = part_rows[4]
        assert A.rsum[gap[1]] == 0
        sets.append([gap[0], gap[1], gap[2]])
        sets.append([gap[1]])
    if n_allele <= MAX_COLUMNS - q:
        sets.append(list(range(n_allele)))
    if MAX_COLUMNS - q + 1 <= len(A.F):
        sets.append(list(range(MAX_COLUMNS - q + 1)))
    return sets


# every (case, model, q, weighted, maxit) whose fits tests/test_hip_assocomni.py compares with the device;
# tests/test_assocomni_host.py asserts the safety conditions for each of them
DEVICE_RUNS = [(case, "additive", CASE_Q[case], False, 25) for case in CASES] + \
    [("n1000", "additive", 12, False, 25), ("n1000", "additive", 29, False, 25), ("n1000", "additive", 0, False, 25),
     ("n257", "dominant", 12, False, 25), ("n257", "recessive", 12, False, 25),
     ("n257", "additive", 12, False, 2), ("n257", "additive", 12, True, 25)]

_CACHE = {}


def reference(case, model, q, weighted=False, maxit=25, dtype=np.float64):
    """glm_sets of a device run, computed once per process and shared (callers do not modify it)."""
    key = (case, model, q, weighted, maxit, np.dtype(dtype).name)
    if key not in _CACHE:
        A, covar, prob, _ = analysis(case, model)
        _CACHE[key] = glm_sets(A.F, run_sets(case, model, q), covar[:q], prob if weighted else None, A.y, maxit, 1e-8, dtype)
    return _CACHE[key]


def gaps(r, want):
    """The three differences of section 23's comparison over the fits without the rank bit: est in units of max(|est|, se),
    se and deviance relative."""
    ok = (want["flags"] & RANK_BIT) == 0
    scale = np.fmax(np.abs(want["coef"]), want["se"])
    with np.errstate(invalid="ignore"):
        return (float(np.nanmax((np.abs(r["coef"] - want["coef"]) / scale)[ok])), float(np.nanmax(np.abs(r["se"] / want["se"] - 1)[ok])),
                float(np.nanmax(np.abs(r["deviance"] / want["deviance"] - 1)[ok])))


def tolerance(case, model, q, weighted=False, maxit=25):
    """100 x the largest float64-versus-longdouble difference of the restatement over the run's fits, at least 1e-12."""
    r, rl = reference(case, model, q, weighted, maxit), reference(case, model, q, weighted, maxit, np.longdouble)
    assert np.array_equal(r["flags"], rl["flags"]) and np.array_equal(r["iterations"], rl["iterations"])
    assert np.array_equal(r["df_h"], rl["df_h"]) and np.array_equal(np.isnan(r["coef"]), np.isnan(rl["coef"]))
    return max(100.0 * max(gaps(r, rl)), 1e-12)


def hla_of(case, without=()):
    """The case's cohort as hlaAssocOmnibus takes it: (hla with ``prob``, y, groups, covar [n, 29]); ``without`` names
    partitions to leave out (the stepwise scan is tested without ``p3b``: it ties with ``p3`` in exact arithmetic, so rounding
    would pick between them)."""
    import hibag_amd as hb
    n, n_allele, seed, extra = CASES[case]
    a1, a2, y, g, covar, prob = cohort(n, n_allele, seed, extra)
    hla, names, _ = AR.hla_of(a1, a2, prob, n_allele, locus="DRB1")
    pn, levels, _ = partitions(n_allele, extra)
    keep = [i for i, nm in enumerate(pn) if nm not in without]
    return hla, y, hb.HlaAlleleGroups(names, [pn[i] for i in keep], [levels[i] for i in keep], g[keep]), covar.T
