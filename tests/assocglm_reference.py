"""CPU restatement of hlaAssocGlm for the tests: DESIGN.md section 23 items 1-7 in numpy, written from the definitions.

Dtype-generic: every function takes ``dtype`` (``numpy.float64`` or ``numpy.longdouble``) and does all its arithmetic in it,
with a Cholesky factorisation and triangular solves of its own (numpy's ``linalg`` takes no longdouble).  ``fit`` is one
IRLS fit, ``assoc_glm`` what ``hibag_hip_assoc_glm`` returns (the fits of all tests and the base model, by slot), ``Backend``
the same behind the interface ``hibag_amd.assocglm`` drives, so that ``hlaAssocGlm`` itself runs on the restatement.  The
samples, tests and feature rows are those of tests/assoc_reference.py."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
from assoc_reference import allele_names, kept_columns       # noqa: F401  (the tests reach them through this module)

MODELS = AR.MODELS
SLOTS, COV0, MAX_COVAR = 16, 3, 12
MAXIT_BIT, RANK_BIT, BOUNDARY_BIT = 1, 2, 4


def cholesky(A, dtype, scale=None, pivots=None):
    """L (lower, L L' = A) column by column, or None where a pivot is <= 1e-11 scale_j; ``scale`` is the diagonal of A unless
    given (the Cox fits give the diagonal before the cancellation).  ``pivots``: a list that receives every tested pivot as
    (pivot, threshold) in float."""
    p = len(A)
    L = np.zeros((p, p), dtype)
    for j in range(p):
        d = A[j, j]
        for m in range(j):
            d = d - L[j, m] * L[j, m]
        limit = dtype(1e-11) * (A[j, j] if scale is None else scale[j])
        if pivots is not None:
            pivots.append((float(d), float(limit)))
        if not d > limit:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, p):
            v = A[i, j]
            for m in range(j):
                v = v - L[i, m] * L[j, m]
            L[i, j] = v / L[j, j]
    return L


def solve(L, b, dtype):
    """beta of L L' beta = b."""
    p = len(b)
    u = np.zeros(p, dtype)
    for i in range(p):
        v = b[i]
        for m in range(i):
            v = v - L[i, m] * u[m]
        u[i] = v / L[i, i]
    for i in range(p - 1, -1, -1):
        v = u[i]
        for m in range(i + 1, p):
            v = v - L[m, i] * u[m]
        u[i] = v / L[i, i]
    return u


def inverse_diagonal(L, dtype):
    """diag((L L')^-1): the squared norms of the columns of L^-1."""
    p = len(L)
    out = np.zeros(p, dtype)
    for j in range(p):
        x = np.zeros(p, dtype)
        for i in range(j, p):
            v = dtype(1) if i == j else dtype(0)
            for m in range(j, i):
                v = v - L[i, m] * x[m]
            x[i] = v / L[i, i]
        out[j] = (x * x).sum()
    return out


def _mean(eta, dtype):
    eps = dtype(2.0) ** -52
    with np.errstate(over="ignore"):
        t = np.exp(eta)
    t = np.where(eta < -30, eps, np.where(eta > 30, 1 / eps, t)).astype(dtype)
    return t, t / (1 + t)


def _deviance(mu, y, wt):
    return (2 * wt * np.log(1 / np.where(y == 1, mu, 1 - mu))).sum()


def fit(X, y, wt, maxit=25, epsilon=1e-8, dtype=np.float64):
    """One fit of items 3-5: dict coef, se [p], deviance, iterations, flags, crit (every iteration's), pivots (every tested
    pivot with its threshold) and eta_max (the largest |eta| the weights of an iteration were taken at)."""
    X = np.asarray(X, dtype)
    y = np.asarray(y, dtype)
    wt = np.asarray(wt, dtype)
    eps = dtype(2.0) ** -52
    p = X.shape[1]
    nan = np.full(p, np.nan)
    mu = (wt * y + dtype(0.5)) / (wt + 1)
    eta = np.log(mu / (1 - mu))
    devold = _deviance(mu, y, wt)
    crits, pivots, eta_max = [], [], 0.0
    flags = 0
    for k in range(1, maxit + 1):
        eta_max = max(eta_max, float(np.abs(eta[wt > 0]).max(initial=0.0)))
        t, mu = _mean(eta, dtype)
        g = np.where(np.abs(eta) > 30, eps, t / ((1 + t) * (1 + t)))
        v = mu * (1 - mu)
        z = eta + (y - mu) / g
        W = wt * (g * g) / v
        A = X.T @ (X * W[:, None])
        b = X.T @ (W * z)
        L = cholesky(A, dtype, pivots=pivots)
        if L is None:
            return dict(coef=nan, se=nan, deviance=np.nan, iterations=k, flags=RANK_BIT, crit=crits, pivots=pivots, eta_max=eta_max)
        beta = solve(L, b, dtype)
        eta = X @ beta
        _, mu = _mean(eta, dtype)
        dev = _deviance(mu, y, wt)
        crit = abs(dev - devold) / (abs(dev) + dtype(0.1))
        crits.append(float(crit))
        if crit < epsilon:
            break
        devold = dev
    else:
        flags |= MAXIT_BIT
    if ((mu < 10 * eps) | (mu > 1 - 10 * eps)).any():
        flags |= BOUNDARY_BIT
    return dict(coef=beta, se=np.sqrt(inverse_diagonal(L, dtype)), deviance=dev, iterations=k, flags=flags, crit=crits, pivots=pivots,
                eta_max=eta_max)


def fit_slots(F, rsum, model, n):
    """Per test the feature rows behind slots 1 and 2 (-1: unused), or None for a test that is not fitted (item 6)."""
    out = []
    T = len(rsum) // 2 if model == "genotype" else len(rsum)
    for t in range(T):
        if model == "genotype":
            het, hom = int(rsum[2 * t]), int(rsum[2 * t + 1])
            out.append(None if (het == 0 and hom == 0) or het + hom == n else (2 * t if het else -1, 2 * t + 1 if hom else -1))
        else:
            top = (2 if model == "additive" else 1) * n
            out.append(None if int(rsum[t]) in (0, top) else (t, -1))
    return out


def glm_rows(F, model, covar, weight, y, maxit=25, epsilon=1e-8, dtype=np.float64):
    """What hibag_hip_assoc_glm returns from the feature rows F [rows, n]: dict of coef, se [T + 1, 16] by slot (float64),
    deviance, iterations, flags [T + 1], and crit, pivots, eta_max, lists of every fit's criteria, tested pivots and largest
    |eta|; fit T is the base model."""
    n = F.shape[1]
    covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
    q = len(covar)
    assert q <= MAX_COVAR
    wt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    slots = fit_slots(F, F.sum(axis=1), model, n) + [(-1, -1)]
    n_fit = len(slots)
    out = dict(coef=np.full((n_fit, SLOTS), np.nan), se=np.full((n_fit, SLOTS), np.nan), deviance=np.full(n_fit, np.nan),
               iterations=np.zeros(n_fit, np.int32), flags=np.zeros(n_fit, np.int32), crit=[[] for _ in range(n_fit)],
               pivots=[[] for _ in range(n_fit)], eta_max=[0.0] * n_fit)
    for f, rows in enumerate(slots):
        if rows is None:
            out["flags"][f] = RANK_BIT
            continue
        used = [0] + [1 + i for i, r in enumerate(rows) if r >= 0] + list(range(COV0, COV0 + q))
        cols = [np.ones(n)] + [F[r].astype(np.float64) for r in rows if r >= 0] + list(covar)
        res = fit(np.stack(cols, axis=1), y, wt, maxit, epsilon, dtype)
        out["coef"][f, used] = np.asarray(res["coef"], np.float64)
        out["se"][f, used] = np.asarray(res["se"], np.float64)
        out["deviance"][f] = float(res["deviance"])
        out["iterations"][f], out["flags"][f], out["crit"][f] = res["iterations"], res["flags"], res["crit"]
        out["pivots"][f], out["eta_max"][f] = res["pivots"], res["eta_max"]
    return out


def assoc_glm(a1, a2, y, n_allele, group_of, model, covar=None, weight=None, maxit=25, epsilon=1e-8, dtype=np.float64):
    """glm_rows for the cohort as hibag_hip_assoc_new takes it; covar [q, n_kept] and weight [n_kept] over the kept samples."""
    A = AR.Analysis(a1, a2, y, n_allele, group_of, model)
    return glm_rows(A.F, model, covar, weight, A.y, maxit, epsilon, dtype)


class Backend(AR.Backend):
    """The restatement behind the interface of hibag_amd.assocglm._DeviceGlm (``hlaAssocGlm(..., _backend=Backend)``)."""

    def glm(self, covar, weight, maxit, epsilon):
        r = glm_rows(self.A.F, self.model, covar, weight, self.A.y, maxit, epsilon, self.dtype)
        return r["coef"], r["se"], r["deviance"], r["iterations"], r["flags"]


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
# (samples, alleles, covariates, seed, with a partition whose level 1 is empty): the sample counts straddle a 256-sample
# boundary of the device's walk (eight waves of four samples per step, and the handle's padding to 128)
CASES = {"n40": (40, 6, 0, 1, False), "n255": (255, 12, 1, 2, False), "n256": (256, 12, 5, 3, False),
         "n257": (257, 12, 12, 4, False), "n1000": (1000, 20, 6, 5, True)}


def cohort(n, n_allele, q, seed, partition=False):
    """(a1, a2, y, group_of or None, covar [q, n], prob [n]): alleles drawn from frequencies ~ 0.75^k, y from a logistic
    model with the effects of alleles 0 and 1 and of the covariates, three samples with an unknown allele, ``prob``
    uniform on (0.3, 1) with two zeros."""
    rng = np.random.default_rng(seed)
    w = 0.75 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    covar = rng.standard_normal((q, n))
    gamma = rng.uniform(-0.5, 0.5, q) / np.sqrt(max(q, 1))
    eta = -0.3 + 0.8 * (a == 0).any(axis=1) - 0.7 * (a == 1).any(axis=1) + gamma @ covar
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    a[rng.choice(n, 3, replace=False), rng.integers(0, 2, 3)] = AR.NA_INTEGER
    prob = rng.uniform(0.3, 1.0, n)
    prob[rng.choice(n, 2, replace=False)] = 0.0
    g = AR.gap_partition(n_allele) if partition else None
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), y, g, covar, prob


def hla_of(case):
    """The case's cohort as hlaAssocGlm takes it: (hla with ``prob``, y, groups or None, covar [n, q])."""
    n, n_allele, q, seed, partition = CASES[case]
    a1, a2, y, g, covar, prob = cohort(n, n_allele, q, seed, partition)
    hla, _, groups = AR.hla_of(a1, a2, prob, n_allele, g)
    return hla, y, groups, covar.T


_CACHE = {}


def reference(case, model, weighted=False, maxit=25, dtype=np.float64):
    """assoc_glm of a case, computed once per process and shared (callers do not modify it)."""
    key = (case, model, weighted, maxit, np.dtype(dtype).name)
    if key not in _CACHE:
        n, n_allele, q, seed, partition = CASES[case]
        a1, a2, y, g, covar, prob = cohort(n, n_allele, q, seed, partition)
        covar, prob = kept_columns(a1, a2, covar, prob)
        _CACHE[key] = assoc_glm(a1, a2, y, n_allele, g, model, covar, prob if weighted else None, maxit, 1e-8, dtype)
    return _CACHE[key]


# every (case, model, weighted, maxit) whose fits tests/test_hip_assocglm.py compares with the device; tests/test_assocglm_host.py
# asserts the safety condition (no convergence criterion within 1e-6 relative of epsilon) for each of them
DEVICE_RUNS = [(case, model, False, 25) for case in CASES for model in MODELS] + \
    [("n257", model, False, 2) for model in MODELS] + [("n257", model, True, 25) for model in MODELS] + \
    [("n40", "genotype", True, 25)]


def tolerance(case, model, weighted=False, maxit=25):
    """100 x the largest float64-versus-longdouble difference of the restatement over the run's fits without the rank bit
    (est in units of max(|est|, se); se and deviance relative), at least 1e-12."""
    r, rl = reference(case, model, weighted, maxit), reference(case, model, weighted, maxit, np.longdouble)
    ok = (r["flags"] & RANK_BIT) == 0
    assert np.array_equal(r["flags"], rl["flags"]) and np.array_equal(r["iterations"], rl["iterations"])
    scale = np.fmax(np.abs(rl["coef"]), rl["se"])
    gaps = [np.nanmax(np.abs(r["coef"] - rl["coef"])[ok] / scale[ok]), np.nanmax(np.abs(r["se"] / rl["se"] - 1)[ok]),
            np.nanmax(np.abs(r["deviance"] / rl["deviance"] - 1)[ok])]
    return max(100.0 * float(max(gaps)), 1e-12)
