"""CPU reference of hlaPredictGroups for the tests: the contract of DESIGN.md section 17 restated in numpy and applied to a
posterior matrix [n_samp, n_cell] (the oracle's, or ``hlaPredict(type="response+prob")``'s).

Only the ORDER of the additions is the definition, so the bin sums and the group dosages are formed by a sequential loop over
the cells in cell order, one plain FP64 addition per cell and target (vectorised over the samples, never over the cells):
``np.sum`` adds pairwise and ``np.add.at`` groups as it likes, neither is used.  ``groups_from_postprob`` is the definition;
``groups`` runs the oracle first; ``relabelled`` is what a user has without the feature: the allele-level call relabelled."""

from __future__ import annotations

import numpy as np

from oracle import oracle as O

NA_INTEGER = -2147483648
KEYS = ("g1", "g2", "prob")
THREADS = 8


def cell_pairs(n_hla: int):
    """(h1, h2) of every cell in cell order: c = h2 + h1 (2 n - h1 - 1) / 2, h1 <= h2."""
    h1, h2 = np.triu_indices(n_hla)
    return h1.astype(np.int64), h2.astype(np.int64)


def levels_of(group_of: np.ndarray) -> np.ndarray:
    """G_q = the largest id + 1 of every partition."""
    return np.asarray(group_of).max(axis=1).astype(np.int64) + 1


def one_partition(pp: np.ndarray, n_hla: int, m: np.ndarray, want_dosage: bool = True) -> dict:
    """The definition for one partition ``m`` [n_hla]: g1, g2 (int32), prob [n_samp]; dosage [n_samp, G]."""
    pp = np.asarray(pp, np.float64)
    ns, P = pp.shape
    m = np.asarray(m, np.int64)
    G = int(m.max()) + 1
    h1, h2 = cell_pairs(n_hla)
    assert P == len(h1)
    a, b = np.minimum(m[h1], m[h2]), np.maximum(m[h1], m[h2])
    bin_of = b + a * (2 * G - a - 1) // 2
    n_bin = G * (G + 1) // 2
    B = np.zeros((n_bin, ns))                                 # +0.0
    D = np.zeros((G, ns))
    cols = np.ascontiguousarray(pp.T)
    with np.errstate(invalid="ignore"):
        for c in range(P):                                    # increasing cell order: the definition
            B[bin_of[c]] += cols[c]
            if not want_dosage:
                continue
            if a[c] == b[c]:
                D[a[c]] += 2 * cols[c]                        # (exact)
            else:
                D[a[c]] += cols[c]
                D[b[c]] += cols[c]
        best = np.zeros(ns)
        won = np.full(ns, -1, np.int64)
        for k in range(n_bin):                                # the first bin with best < B strictly, in bin order
            up = best < B[k]                                  # (False for a NaN sum)
            best = np.where(up, B[k], best)
            won = np.where(up, k, won)
    ga, gb = np.triu_indices(G)                               # bin order IS the cell order of a G-allele model
    ok = won >= 0
    w = np.where(ok, won, 0)
    out = {"g1": np.where(ok, ga[w], NA_INTEGER).astype(np.int32), "g2": np.where(ok, gb[w], NA_INTEGER).astype(np.int32),
           "prob": np.where(ok, best, 0.0)}
    if want_dosage:
        out["dosage"] = np.ascontiguousarray(D.T)
    return out


def groups_from_postprob(postprob: np.ndarray, n_hla: int, group_of: np.ndarray, want_dosage: bool = True) -> dict:
    """The definition.  ``postprob`` [n_samp, n_cell] sample-major, ``group_of`` [n_part, n_hla]: g1, g2, prob
    [n_samp, n_part] and dosage [n_samp, sum of G_q].  Equal rows of ``group_of`` are computed once."""
    group_of = np.asarray(group_of)
    assert group_of.ndim == 2 and group_of.shape[1] == n_hla
    done = {}
    parts = []
    for row in group_of:
        key = row.tobytes()
        if key not in done:
            done[key] = one_partition(postprob, n_hla, row, want_dosage)
        parts.append(done[key])
    out = {k: np.ascontiguousarray(np.stack([p[k] for p in parts], axis=1)) for k in KEYS}
    if want_dosage:
        out["dosage"] = np.ascontiguousarray(np.concatenate([p["dosage"] for p in parts], axis=1))
    return out


def groups(model, G, group_of, vote: int = 1, want_dosage: bool = True, avx2: bool = True) -> dict:
    """The oracle's prediction of every sample of G (int32 [n_samp, n_snp]) and the group calls from its posterior matrix;
    ``call``: the oracle's own h1, h2, prob, dosage; ``postprob``: its matrix."""
    G = np.ascontiguousarray(G, np.int32)
    r = O.predict(O.flatten(model), G, vote_method=vote, want_dosage=True, want_prob=True, avx2=avx2,
                  n_threads=THREADS if avx2 else 1)
    out = groups_from_postprob(r["postprob"], int(model.n_hla), group_of, want_dosage)
    out["matching"] = r["matching"]
    out["call"] = {k: r[k] for k in ("h1", "h2", "prob", "dosage")}
    out["postprob"] = r["postprob"]
    return out


def relabelled(h1: np.ndarray, h2: np.ndarray, m: np.ndarray):
    """The allele-level call (h1, h2) relabelled with the partition ``m``: (min, max) of the two groups, NA stays NA."""
    m = np.asarray(m, np.int64)
    ok = h1 != NA_INTEGER
    a, b = m[np.where(ok, h1, 0)], m[np.where(ok, h2, 0)]
    return (np.where(ok, np.minimum(a, b), NA_INTEGER).astype(np.int32), np.where(ok, np.maximum(a, b), NA_INTEGER).astype(np.int32))


def assert_groups_equal(got, want, what="", keys=KEYS + ("matching", "dosage")):
    """Every entry of every key equal (NaN == NaN); the message names the first differing (sample, column)."""
    for key in keys:
        if key == "dosage" and got.get("dosage") is None:
            continue
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            continue
        bad = (a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a != b
        at = np.argwhere(bad)
        first = tuple(int(v) for v in at[0])
        raise AssertionError(f"{what} {key}: {len(at)} entries differ, the first at {first}: "
                             f"got {a[first]!r}, reference {b[first]!r}")
