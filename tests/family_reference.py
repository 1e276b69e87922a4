"""CPU reference of hlaPredictFamily for the tests: the contract of DESIGN.md section 19 restated in numpy and applied to a
posterior matrix [n_samp, n_cell] (the oracle's, or ``hlaPredict(type="response+prob")``'s).

Only the ORDER of the operations is the definition.  The support and the dosages are formed by a sequential loop over the
cells in cell order, one plain FP64 addition per cell and target (vectorised over the samples of one depth, never over the
cells): ``np.sum`` adds pairwise and ``np.add.at`` groups as it likes, neither is used.  The weight of a cell is two
multiplications, one addition, an exact halving and one multiplication, as separate numpy operations (numpy fuses nothing).
Samples are finished depth by depth, so a parent's (D, S) exists when its children need it.  ``family_from_postprob`` is the
definition; ``family`` runs the oracle first.  (A NaN weight sum, the poisoned batch of the contract's rule 4, exists on the
device only -- the library repairs it before a host array is written -- and is not restated here.)"""

from __future__ import annotations

import numpy as np

from given_reference import NA_INTEGER, assert_given_equal, cell_pairs, conditional  # noqa: F401  (conditional: rule 7)
from oracle import oracle as O

KEYS = ("h1", "h2", "prob", "support")
THREADS = 8


def depths(pedigree: np.ndarray) -> np.ndarray:
    """depth [n_samp] of a pedigree whose parents precede their children (asserted): 0 without a parent in the call, else
    1 + the larger depth of its parents."""
    ped = np.asarray(pedigree, np.int64)
    assert ped.ndim == 2 and ped.shape[1] == 2, ped.shape
    d = np.zeros(len(ped), np.int64)
    for s in range(len(ped)):
        for p in ped[s]:
            assert -1 <= p < s, (s, p)
            if p >= 0:
                d[s] = max(d[s], d[p] + 1)
    return d


def family_from_postprob(postprob: np.ndarray, n_hla: int, pedigree: np.ndarray, prior=None) -> dict:
    """The definition.  ``postprob`` [n_samp, n_cell] sample-major; ``pedigree`` int [n_samp, 2], parents before children;
    ``prior`` float [n_hla] or None: h1, h2 (int32), prob (joint), support [n_samp] and dosage [n_samp, n_hla] (joint)."""
    pp = np.asarray(postprob, np.float64)
    ns, P = pp.shape
    ped = np.asarray(pedigree, np.int64)
    assert ped.shape == (ns, 2)
    depth = depths(ped)
    q = None if prior is None else np.asarray(prior, np.float64)
    assert q is None or (q.shape == (n_hla,) and np.all(np.isfinite(q) & (q > 0)))
    h1, h2 = cell_pairs(n_hla)
    assert P == len(h1)
    D = np.zeros((ns, n_hla))
    S = np.zeros(ns)
    best_all, won_all = np.zeros(ns), np.full(ns, -1, np.int64)
    with np.errstate(all="ignore"):
        for d in np.unique(depth):                                # ascending
            idx = np.nonzero(depth == d)[0]
            R = np.ones((2, n_hla, len(idx)))                      # rule 1: unknown parents keep 1.0
            for k in (0, 1):
                p = ped[idx, k]
                Sp = np.where(p >= 0, S[np.maximum(p, 0)], 0.0)
                use = (p >= 0) & (Sp > 0)                          # (False for a NaN support)
                r = 0.5 * (D[p[use]].T / Sp[use])                  # one division, an exact halving
                if q is not None:
                    r = r / q[:, None]
                R[k][:, use] = r
            rf, rm = R[0], R[1]
            cols = np.ascontiguousarray(pp[idx].T)
            support = np.zeros(len(idx))                           # +0.0
            best = np.zeros(len(idx))
            won = np.full(len(idx), -1, np.int64)
            Dd = np.zeros((n_hla, len(idx)))
            for c in range(P):                                     # increasing cell order: the definition
                i, j = h1[c], h2[c]
                a = rf[i] * rm[j]
                b = rf[j] * rm[i]
                w = 0.5 * (a + b)
                x = cols[c] * w                                    # rule 2
                support = support + x                              # rule 3
                up = best < x                                      # rule 4 (False for a NaN x)
                best = np.where(up, x, best)
                won = np.where(up, c, won)
                if i == j:                                         # rule 5
                    Dd[i] = Dd[i] + 2 * x                          # (2 x is exact)
                else:
                    Dd[i] = Dd[i] + x
                    Dd[j] = Dd[j] + x
            S[idx], D[idx] = support, Dd.T
            best_all[idx], won_all[idx] = best, won
    ok = won_all >= 0
    w = np.where(ok, won_all, 0)
    return {"h1": np.where(ok, h1[w], NA_INTEGER).astype(np.int32), "h2": np.where(ok, h2[w], NA_INTEGER).astype(np.int32),
            "prob": np.where(ok, best_all, 0.0), "support": S, "dosage": D}


def family(model, G, pedigree, prior=None, vote: int = 1, avx2: bool = True) -> dict:
    """The oracle's prediction of every sample of G (int32 [n_samp, n_snp]) and the family calls from its posterior matrix;
    ``call``: the oracle's own h1, h2, prob, dosage; ``postprob``: its matrix."""
    G = np.ascontiguousarray(G, np.int32)
    r = O.predict(O.flatten(model), G, vote_method=vote, want_dosage=True, want_prob=True, avx2=avx2,
                  n_threads=THREADS if avx2 else 1)
    out = family_from_postprob(r["postprob"], int(model.n_hla), pedigree, prior)
    out["matching"] = r["matching"]
    out["call"] = {k: r[k] for k in ("h1", "h2", "prob", "dosage")}
    out["postprob"] = r["postprob"]
    return out


def founders_only(n_samp: int) -> np.ndarray:
    return np.full((n_samp, 2), -1, np.int32)


def model_prior(model) -> np.ndarray:
    """The prior the classifiers carry, written out here independently of the package's hlaModelAllelePrior."""
    n = int(model.n_hla)
    q = np.zeros(n)
    for c in model.classifiers:
        own = np.zeros(n)                                     # the classifier's summed frequencies, in haplotype order
        for h, f in zip(np.asarray(c.hla), np.asarray(c.freq, np.float64)):
            own[int(h)] += f
        q = q + own
    q = q / len(model.classifiers)
    return np.where(q > 0, q, 1.0)


def correct_pairs(res: dict, truth: np.ndarray, idx=None) -> int:
    """How many of the samples `idx` (default: all) are called with their true sorted pair."""
    idx = np.arange(len(truth)) if idx is None else np.asarray(idx)
    return int(np.count_nonzero((res["h1"][idx] == truth[idx, 0]) & (res["h2"][idx] == truth[idx, 1])))


assert_family_equal = assert_given_equal
