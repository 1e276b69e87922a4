"""CPU reference of hlaGenoLD / hlaLDMatrix (hibag_amd/ld.py) for the tests.

The integer sums come from float64 BLAS products (exact: every partial sum is an integer below 2^53), the r^2 formula
from numpy element-wise operations with the same single roundings as the device:
    num = n Sxy - Sx Sy, dx = n Sxx - Sx^2, dy = n Syy - Sy^2 (int64);  r2 = (num * num) / (dx * dy) in double, NaN if dx or dy is 0.
"""

from __future__ import annotations

from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np

NA = -2147483648


def r2_formula(n, sxy, sx, sy, sxx, syy):
    n, sxy, sx, sy, sxx, syy = (np.asarray(v, np.int64) for v in (n, sxy, sx, sy, sxx, syy))
    num = n * sxy - sx * sy
    dx = n * sxx - sx * sx
    dy = n * syy - sy * sy
    a = num.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = (a * a) / (dx.astype(np.float64) * dy.astype(np.float64))
    return np.where((dx == 0) | (dy == 0), np.nan, r2)


def r2_exact(n, sxy, sx, sy, sxx, syy) -> Optional[Fraction]:
    n, sxy, sx, sy, sxx, syy = (int(v) for v in (n, sxy, sx, sy, sxx, syy))
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    return None if dx == 0 or dy == 0 else Fraction(num * num, dx * dy)


def hla_indices(allele1: Sequence, allele2: Sequence) -> Tuple[List[str], np.ndarray, np.ndarray]:
    alleles = sorted({a for a in list(allele1) + list(allele2) if a is not None})
    pos = {a: i for i, a in enumerate(alleles)}
    i1 = np.array([NA if (a is None or b is None) else pos[a] for a, b in zip(allele1, allele2)], np.int64)
    i2 = np.array([NA if (a is None or b is None) else pos[b] for a, b in zip(allele1, allele2)], np.int64)
    return alleles, i1, i2


def geno_ld_sums(geno: np.ndarray, i1: np.ndarray, i2: np.ndarray, n_allele: int):
    """The six integer sums of hlaGenoLD per (SNP, allele), int64 [n_snp, n_allele] each."""
    g = np.asarray(geno)
    valid = (g == 0) | (g == 1) | (g == 2)
    X = np.where(valid, g, 0).astype(np.float64)
    M = valid.astype(np.float64)
    V = ((i1 != NA) & (i2 != NA)).astype(np.float64)
    a = np.arange(n_allele)
    Y = ((i1[:, None] == a[None, :]).astype(np.float64) + (i2[:, None] == a[None, :])) * V[:, None]
    n = (M @ V)[:, None]
    sx = (X @ V)[:, None]
    sxx = ((X * X) @ V)[:, None]
    sy, syy, sxy = M @ Y, M @ (Y * Y), X @ Y
    shape = (g.shape[0], n_allele)
    return tuple(np.broadcast_to(np.rint(v).astype(np.int64), shape) for v in (n, sxy, sx, sy, sxx, syy))


def geno_ld(geno: np.ndarray, allele1: Sequence, allele2: Sequence):
    """(ld [n_snp], r2 [n_snp, n_allele], alleles): the mean sums the non-NaN r^2 sequentially in allele order."""
    alleles, i1, i2 = hla_indices(allele1, allele2)
    sums = geno_ld_sums(geno, i1, i2, len(alleles))
    r2 = r2_formula(*sums)
    s = np.zeros(r2.shape[0])
    cnt = np.zeros(r2.shape[0], np.int64)
    for k in range(r2.shape[1]):
        ok = ~np.isnan(r2[:, k])
        s = s + np.where(ok, r2[:, k], 0.0)
        cnt += ok
    with np.errstate(divide="ignore", invalid="ignore"):
        ld = np.where(cnt > 0, s / cnt, np.nan)
    return ld, r2, alleles


def ld_matrix(geno: np.ndarray):
    """cor(t(geno), use = "na.or.complete")^2 by the formula: (r2 [k, k], complete-sample count)."""
    g = np.asarray(geno)
    k = g.shape[0]
    valid = (g == 0) | (g == 1) | (g == 2)
    complete = valid.all(axis=0)
    n = int(complete.sum())
    if k == 0:
        return np.empty((0, 0)), n
    if n < 2:
        return np.full((k, k), np.nan), n
    X = g[:, complete].astype(np.float64)
    G = np.rint(X @ X.T).astype(np.int64)
    sx = np.rint(X.sum(axis=1)).astype(np.int64)
    sxx = np.rint((X * X).sum(axis=1)).astype(np.int64)
    r2 = r2_formula(n, G, sx[:, None], sx[None, :], sxx[:, None], sxx[None, :])
    np.fill_diagonal(r2, 1.0)
    return r2, n


def maf_keep(geno: np.ndarray, maf: float) -> np.ndarray:
    """hlaLDMatrix's MAF filter: indices of the kept SNPs."""
    g = np.asarray(geno)
    if np.isnan(maf) or maf <= 0:
        return np.arange(g.shape[0])
    valid = (g == 0) | (g == 1) | (g == 2)
    s = np.where(valid, g, 0).sum(axis=1)
    nv = valid.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = (s / nv) * 0.5
        af = np.minimum(af, 1.0 - af)
        return np.flatnonzero(af >= maf)


# ---- literal restatements of R's cor(...)^2 (centred sums, as stats::cor computes a Pearson correlation) ----

def _cor(x: np.ndarray, y: np.ndarray) -> float:
    xm, ym = x - x.mean(), y - y.mean()
    sxx, syy = float(xm @ xm), float(ym @ ym)
    if sxx == 0 or syy == 0:
        return np.nan
    return float(xm @ ym) / np.sqrt(sxx * syy)


def geno_ld_literal(geno: np.ndarray, allele1: Sequence, allele2: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """mean(cor(x, allele.mat, use = "pairwise.complete.obs")^2, na.rm = TRUE) per SNP, and the r^2 matrix."""
    alleles, i1, i2 = hla_indices(allele1, allele2)
    A = len(alleles)
    usable = (i1 != NA) & (i2 != NA)
    a = np.arange(A)
    Y = (i1[:, None] == a[None, :]).astype(np.float64) + (i2[:, None] == a[None, :])
    g = np.asarray(geno)
    ld = np.full(g.shape[0], np.nan)
    r2 = np.full((g.shape[0], A), np.nan)
    for j in range(g.shape[0]):
        use = usable & ((g[j] == 0) | (g[j] == 1) | (g[j] == 2))
        x = g[j, use].astype(np.float64)
        if x.size < 2:
            continue
        for k in range(A):
            c = _cor(x, Y[use, k])
            r2[j, k] = c * c
        ok = ~np.isnan(r2[j])
        if ok.any():
            ld[j] = np.mean(r2[j, ok])
    return ld, r2


def ld_matrix_literal(geno: np.ndarray) -> np.ndarray:
    g = np.asarray(geno)
    k = g.shape[0]
    valid = (g == 0) | (g == 1) | (g == 2)
    complete = valid.all(axis=0)
    out = np.full((k, k), np.nan)
    if complete.sum() < 2:
        return out
    X = g[:, complete].astype(np.float64)
    for i in range(k):
        for j in range(i + 1, k):
            c = _cor(X[i], X[j])
            out[i, j] = out[j, i] = c * c
        out[i, i] = 1.0
    return out
