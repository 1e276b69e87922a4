"""Plain-loop restatement of the arithmetic of a merge of k models' posteriors (``hlaPredMerge``, R/HIBAG.R:958-1019 with
HIBAG_SumList, HIBAG_UpdateAddProbW and HIBAG_NormalizeProb), one sample at a time over Python floats (IEEE float64, no
fused multiply-add, no vectorised reduction whose order numpy chooses).  The yardstick of the tests of ``hlaPredictMerge``;
it uses neither ``hibag_amd.merge`` nor the library.  The names are not its business: the caller says which merged row
each source cell goes to.

Merged row (i, j), i <= j, of n merged alleles sits at ``j + i (2 n - i - 1) / 2`` and is named ``allele[j]/allele[i]``:
its first name is j, its second i.
"""

import math

import numpy as np


def normalised_weights(weight, k):
    """Step 1: w = weight / sum(weight) in float64, 1 / k each by default."""
    if weight is None:
        return [1.0 / k] * k
    total = 0.0
    for x in weight:
        total += float(x)
    return [float(x) / total for x in weight]


def merge_reference(postprobs, matchings, weight, row_of_cell, n_hla, use_matching=True):
    """``postprobs[i]`` float64 [n_cell_i, n_samp], ``matchings[i]`` [n_samp], ``row_of_cell[i]`` [n_cell_i] -> merged row.
    Returns ``h1``, ``h2``, ``prob``, ``matching``, ``dosage`` [n_hla, n_samp], ``postprob`` [P, n_samp]."""
    k = len(postprobs)
    n_samp = np.asarray(postprobs[0]).shape[1]
    P = n_hla * (n_hla + 1) // 2
    w = normalised_weights(weight, k)
    first_of, second_of = [], []
    for i in range(n_hla):
        for j in range(i, n_hla):
            first_of.append(j)
            second_of.append(i)
    # an allele's rows as first and as second name, ascending: the order its dosage is summed in
    first_rows = [[r for r in range(P) if first_of[r] == a] for a in range(n_hla)]
    second_rows = [[r for r in range(P) if second_of[r] == a] for a in range(n_hla)]
    # gather lists: model order, then ascending source cell
    gather = [[] for _ in range(P)]
    for i in range(k):
        for j, r in enumerate(row_of_cell[i]):
            gather[int(r)].append((i, j))
    out = dict(h1=np.empty(n_samp, np.int32), h2=np.empty(n_samp, np.int32), prob=np.empty(n_samp, np.float64),
               matching=np.empty(n_samp, np.float64), dosage=np.empty((n_hla, n_samp), np.float64),
               postprob=np.empty((P, n_samp), np.float64))
    for s in range(n_samp):
        m = 0.0
        w2 = []
        for i in range(k):                                   # steps 2 and 3
            mi = float(matchings[i][s])
            m += w[i] * mi
            w2.append(w[i] * mi if use_matching else w[i])
        acc = []
        for r in range(P):                                   # step 4
            a = 0.0
            for i, j in gather[r]:
                a += float(postprobs[i][j, s]) * w2[i]
            acc.append(a)
        total = 0.0
        for r in range(P):                                   # step 5
            total += acc[r]
        prob = []
        for r in range(P):
            if total == 0.0 or math.isnan(total) or math.isnan(acc[r]):
                with np.errstate(all="ignore"):                  # (IEEE: 0/0 = NaN, x/0 = inf; Python's floats raise)
                    prob.append(float(np.float64(acc[r]) / np.float64(total)))
            else:
                prob.append(acc[r] / total)
        best, key = 0, -math.inf                             # step 6: first maximum, NaN read as -inf
        for r in range(P):
            x = -math.inf if math.isnan(prob[r]) else prob[r]
            if r == 0 or x > key:
                best, key = r, x
        for a in range(n_hla):                               # step 7
            d1 = 0.0
            for r in first_rows[a]:
                d1 += prob[r]
            d2 = 0.0
            for r in second_rows[a]:
                d2 += prob[r]
            out["dosage"][a, s] = d1 + d2
        out["matching"][s] = m
        out["h2"][s], out["h1"][s] = first_of[best], second_of[best]
        out["prob"][s] = prob[best]
        out["postprob"][:, s] = prob
    return out
