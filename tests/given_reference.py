"""CPU reference of hlaPredictGiven for the tests: the contract of DESIGN.md section 18 restated in numpy and applied to a
posterior matrix [n_samp, n_cell] (the oracle's, or ``hlaPredict(type="response+prob")``'s).

Only the ORDER of the additions is the definition, so the support and the dosages are formed by a sequential loop over the
cells in cell order, one plain FP64 addition per cell and target, selected per sample (vectorised over the samples, never over
the cells): ``np.sum`` adds pairwise and ``np.add.at`` groups as it likes, neither is used.  ``given_from_postprob`` is the
definition; ``given`` runs the oracle first.  (A NaN weight sum, the poisoned batch of the contract's rule 2, exists on the
device only -- the library repairs it before a host array is written -- and is not restated here.)"""

from __future__ import annotations

import numpy as np

from oracle import oracle as O

NA_INTEGER = -2147483648
KEYS = ("h1", "h2", "prob", "support")
THREADS = 8


def cell_pairs(n_hla: int):
    """(h1, h2) of every cell in cell order: c = h2 + h1 (2 n - h1 - 1) / 2, h1 <= h2."""
    h1, h2 = np.triu_indices(n_hla)
    return h1.astype(np.int64), h2.astype(np.int64)


def unpack(allow: np.ndarray, n_hla: int) -> np.ndarray:
    """The C form uint32 [n_samp, 2, W] (allele h = bit h % 32 of word h // 32; bits >= n_hla ignored) or a boolean array
    [n_samp, 2, n_hla] -> bool [n_samp, 2, n_hla].  Written with shifts, not with the package's packer."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        assert a.shape[1:] == (2, n_hla)
        return a
    assert a.dtype == np.uint32 and a.shape[1:] == (2, (n_hla + 31) // 32), (a.dtype, a.shape)
    h = np.arange(n_hla)
    return ((a[:, :, h // 32] >> (h % 32).astype(np.uint32)) & np.uint32(1)).astype(np.bool_)


def pack(allowed: np.ndarray) -> np.ndarray:
    """bool [n_samp, 2, n_hla] -> the C form, written with shifts."""
    allowed = np.asarray(allowed, np.bool_)
    ns, _, n = allowed.shape
    out = np.zeros((ns, 2, (n + 31) // 32), np.uint32)
    for h in range(n):
        out[:, :, h // 32] |= allowed[:, :, h].astype(np.uint32) << np.uint32(h % 32)
    return out


def given_from_postprob(postprob: np.ndarray, n_hla: int, allow: np.ndarray, want_dosage: bool = True) -> dict:
    """The definition.  ``postprob`` [n_samp, n_cell] sample-major, ``allow`` as :func:`unpack` takes it: h1, h2 (int32), prob
    (joint), support [n_samp] and dosage [n_samp, n_hla] (joint)."""
    pp = np.asarray(postprob, np.float64)
    ns, P = pp.shape
    A = unpack(allow, n_hla)
    assert len(A) == ns
    h1, h2 = cell_pairs(n_hla)
    assert P == len(h1)
    cols = np.ascontiguousarray(pp.T)
    inA, inB = np.ascontiguousarray(A[:, 0].T), np.ascontiguousarray(A[:, 1].T)          # [n_hla, n_samp]
    support = np.zeros(ns)                                    # +0.0
    best = np.zeros(ns)
    won = np.full(ns, -1, np.int64)
    D = np.zeros((n_hla, ns))
    with np.errstate(invalid="ignore"):
        for c in range(P):                                    # increasing cell order: the definition
            a, b = h1[c], h2[c]
            ok = (inA[a] & inB[b]) | (inB[a] & inA[b])
            x = cols[c]
            support = np.where(ok, support + x, support)      # the selected add: an inconsistent NaN cell poisons nothing
            up = ok & (best < x)                              # (False for a NaN cell)
            best = np.where(up, x, best)
            won = np.where(up, c, won)
            if not want_dosage:
                continue
            if a == b:
                D[a] = np.where(ok, D[a] + 2 * x, D[a])       # (2 x is exact)
            else:
                D[a] = np.where(ok, D[a] + x, D[a])
                D[b] = np.where(ok, D[b] + x, D[b])
    ok = won >= 0
    w = np.where(ok, won, 0)
    out = {"h1": np.where(ok, h1[w], NA_INTEGER).astype(np.int32), "h2": np.where(ok, h2[w], NA_INTEGER).astype(np.int32),
           "prob": np.where(ok, best, 0.0), "support": support}
    if want_dosage:
        out["dosage"] = np.ascontiguousarray(D.T)
    return out


def conditional(res: dict) -> dict:
    """Rule 5: prob / support and dosage / support, one IEEE division each, where support > 0; the joint values elsewhere."""
    s = res["support"]
    pos = s > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"prob": np.where(pos, res["prob"] / np.where(pos, s, 1.0), res["prob"])}
        if res.get("dosage") is not None:
            out["dosage"] = np.where(pos[:, None], res["dosage"] / np.where(pos, s, 1.0)[:, None], res["dosage"])
    return out


def given(model, G, allow, vote: int = 1, want_dosage: bool = True, avx2: bool = True) -> dict:
    """The oracle's prediction of every sample of G (int32 [n_samp, n_snp]) and the given calls from its posterior matrix;
    ``call``: the oracle's own h1, h2, prob, dosage; ``postprob``: its matrix."""
    G = np.ascontiguousarray(G, np.int32)
    r = O.predict(O.flatten(model), G, vote_method=vote, want_dosage=True, want_prob=True, avx2=avx2,
                  n_threads=THREADS if avx2 else 1)
    out = given_from_postprob(r["postprob"], int(model.n_hla), allow, want_dosage)
    out["matching"] = r["matching"]
    out["call"] = {k: r[k] for k in ("h1", "h2", "prob", "dosage")}
    out["postprob"] = r["postprob"]
    return out


def full_sets(n_samp: int, n_hla: int) -> np.ndarray:
    return np.ones((n_samp, 2, n_hla), np.bool_)


def assert_given_equal(got, want, what="", keys=KEYS + ("matching", "dosage")):
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
