"""CPU reference of hlaDistance (hibag_amd/distance.py) for the tests.

``classifier_matrix`` restates HIBAG_Distance (src/HIBAG.cpp:1284-1332) with numpy: per haplotype pair i <= j the
distance d and f = freq[i] * freq[j] are vectorised, and each cell's two sums are taken with ``np.cumsum``, which adds
sequentially in the reference's i-major order (``np.sum`` adds pairwise and gives other bits).  ``fold`` is R's
``num + !is.na(m); m[is.na(m)] <- 0; Reduce("+", lst) / num`` (R/HIBAG.R:1545-1570), literally.  ``literal_*`` are
line-by-line transliterations (Python floats are IEEE doubles; no step fuses a multiply into an add), the yardstick's
own check.
"""

from __future__ import annotations

import operator
from typing import List, Sequence, Tuple

import numpy as np


def _bits(haplo: Sequence[str], H: int) -> np.ndarray:
    k = len(haplo[0]) if H else 0
    return (np.frombuffer("".join(haplo).encode(), np.uint8).reshape(H, k) == ord("1")).astype(np.float64)


def classifier_matrix(n_hla: int, hla, freq, haplo) -> np.ndarray:
    """One classifier's [n_hla, n_hla] matrix: dist_sum / freq_sum per cell, symmetric, NaN where the cell has no pair
    (and 0/0 where every f underflowed).  Haplotypes must be grouped by ascending allele, as the models here are."""
    hla = np.asarray(hla, np.int64)
    freq = np.asarray(freq, np.float64)
    H = len(hla)
    m = np.full((n_hla, n_hla), np.nan)
    if H == 0:
        return m
    assert np.all(np.diff(hla) >= 0), "haplotypes must be grouped by ascending allele"
    X = _bits(haplo, H)
    d = X @ (1 - X).T + (1 - X) @ X.T                       # exact small integers
    iu, ju = np.triu_indices(H)                             # i-major, j ascending: the reference's loop order
    f = freq[iu] * freq[ju]
    fd = f * d[iu, ju]
    cell = hla[iu] * n_hla + hla[ju]
    order = np.argsort(cell, kind="stable")                 # each cell's pairs together, in loop order
    cs = cell[order]
    uniq, first, counts = np.unique(cs, return_index=True, return_counts=True)
    row = np.repeat(np.arange(len(uniq)), counts)
    pos = np.arange(len(cs)) - np.repeat(first, counts)
    sums = [np.empty(len(uniq)), np.empty(len(uniq))]
    width = np.ceil(np.log2(counts)).astype(np.int64)       # cells of similar length padded together
    for w in np.unique(width):
        cells = np.flatnonzero(width == w)
        sel = np.isin(row, cells)
        slot = np.searchsorted(cells, row[sel])
        for s, v in zip(sums, (f, fd)):
            P = np.zeros((len(cells), int(counts[cells].max())))   # trailing zeros: x + 0.0 == x for these sums (x >= 0)
            P[slot, pos[sel]] = v[order][sel]
            s[cells] = np.cumsum(P, axis=1)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        val = sums[1] / sums[0]
    a, b = uniq // n_hla, uniq % n_hla
    m[a, b] = val
    m[b, a] = val
    return m


def fold(lst: List[np.ndarray]) -> np.ndarray:
    """R's fold over the classifiers' matrices (NaN kept in the input)."""
    num = np.zeros(lst[0].shape, np.int64)
    zero = []
    for m in lst:
        num = num + ~np.isnan(m)
        zero.append(np.where(np.isnan(m), 0.0, m))
    acc = zero[0]
    for z in zero[1:]:
        acc = acc + z
    with np.errstate(divide="ignore", invalid="ignore"):
        return acc / num


def distance(model) -> Tuple[np.ndarray, np.ndarray]:
    """(result [n_hla, n_hla], per-classifier matrices [C, n_hla, n_hla]) of an HlaAttrBagObj."""
    lst = [classifier_matrix(model.n_hla, c.hla, c.freq, c.haplo) for c in model.classifiers]
    return fold(lst), np.stack(lst)


def literal_classifier(num_hla: int, I, freq, haplo) -> np.ndarray:
    """HIBAG_Distance line by line: I are R's 1-based match() indices, the distance a character-by-character comparison."""
    n = len(I)
    freq_sum = [[0.0] * num_hla for _ in range(num_hla)]
    dist_sum = [[0.0] * num_hla for _ in range(num_hla)]
    for i in range(n):
        for j in range(i, n):
            s1, s2 = haplo[i], haplo[j]
            d = sum(map(operator.ne, s1, s2))               # for (; *s1 && *s2; s1++, s2++) if (*s1 != *s2) d++;
            f = float(freq[i]) * float(freq[j])
            fs, ds = freq_sum[I[i] - 1], dist_sum[I[i] - 1]
            fs[I[j] - 1] += f
            ds[I[j] - 1] += f * d
    out = np.empty((num_hla, num_hla))
    for i in range(num_hla):
        for j in range(i, num_hla):
            x, y = dist_sum[i][j], freq_sum[i][j]
            v = x / y if y != 0 else float("nan")           # R: 0/0 is NaN (and x/0 cannot occur: x is 0 when y is)
            out[i, j] = out[j, i] = v
    return out


def literal_distance(model) -> Tuple[np.ndarray, np.ndarray]:
    """hlaDistance (R/HIBAG.R:1545-1570) around literal_classifier."""
    n_hla = len(model.hla_allele)
    num = np.zeros((n_hla, n_hla), np.int64)
    lst, raw = [], []
    for c in model.classifiers:
        m = literal_classifier(n_hla, [int(h) + 1 for h in c.hla], c.freq, c.haplo)
        raw.append(m.copy())
        num = num + ~np.isnan(m)
        m[np.isnan(m)] = 0
        lst.append(m)
    rv = lst[0]
    for m in lst[1:]:                                        # Reduce("+", lst): a left fold from lst[[1]]
        rv = rv + m
    with np.errstate(divide="ignore", invalid="ignore"):
        return rv / num, np.stack(raw)
