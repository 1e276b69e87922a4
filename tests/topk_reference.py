"""CPU reference of hlaPredictTopK for the tests: the k largest cells of the oracle's posterior matrix, per sample.

``select`` is the definition -- per sample ``idx = np.argsort(-col, kind="stable")``, keep those with ``col[idx] > 0``
(NaN and zero drop out), the first k, cell -> pair by the formula of the library's finish (p = h2 + h1 (2n - h1 - 1) / 2,
src/LibHLA.cpp:1523), padded with NA_INTEGER / 0.0.  ``select_fast`` is the form a user writes around
``hlaPredict(type="response+prob")`` and tools/topk_bench.py times: ``np.argpartition``, then an ordered sort of the k
survivors; tests/test_topk_host.py pins the two equal.  ``topk`` runs the oracle and selects."""

from __future__ import annotations

import numpy as np

from oracle import oracle as O

NA_INTEGER = -2147483648
KEYS = ("h1", "h2", "prob")
THREADS = 8


def pair_of_cell(cell: np.ndarray, n_hla: int):
    """(h1, h2), h1 <= h2, of the cells p = h2 + h1 (2 n - h1 - 1) / 2; NA_INTEGER where cell < 0."""
    cell = np.asarray(cell, np.int64)
    h = np.arange(n_hla, dtype=np.int64)
    start = h * (2 * n_hla - h + 1) // 2                     # the first cell of row h1: (h1, h1)
    ok = cell >= 0
    c = np.where(ok, cell, 0)
    h1 = np.searchsorted(start, c, side="right") - 1
    h2 = h1 + c - start[h1]
    return (np.where(ok, h1, NA_INTEGER).astype(np.int32), np.where(ok, h2, NA_INTEGER).astype(np.int32))


def _finish(cell: np.ndarray, val: np.ndarray, k: int, n_hla: int) -> dict:
    """Pads [n, <= k] cells (-1 = none) and values to k ranks and names the pairs."""
    n, have = cell.shape
    if have < k:
        cell = np.concatenate([cell, np.full((n, k - have), -1, cell.dtype)], axis=1)
        val = np.concatenate([val, np.zeros((n, k - have))], axis=1)
    h1, h2 = pair_of_cell(cell, n_hla)
    return {"h1": h1, "h2": h2, "prob": np.where(cell >= 0, val, 0.0)}


def select(postprob: np.ndarray, k: int, n_hla: int) -> dict:
    """The definition.  ``postprob`` [n_samp, n_cell] sample-major (the oracle's / ``predict_raw``'s); returns h1, h2
    (int32) and prob, each [n_samp, k]."""
    pp = np.asarray(postprob, np.float64)
    assert pp.ndim == 2 and pp.shape[1] == n_hla * (n_hla + 1) // 2 and k >= 1
    cells, vals = [], []
    for col in pp:
        idx = np.argsort(-col, kind="stable")
        idx = idx[col[idx] > 0][:k]
        cells.append(np.concatenate([idx, np.full(k - len(idx), -1, idx.dtype)]))
        vals.append(np.concatenate([col[idx], np.zeros(k - len(idx))]))
    cell = np.stack(cells) if cells else np.zeros((0, k), np.int64)
    val = np.stack(vals) if vals else np.zeros((0, k))
    return _finish(cell, val, k, n_hla)


def select_fast(postprob: np.ndarray, k: int, n_hla: int) -> dict:
    """The same lists by ``np.argpartition`` and an ordered sort of the k survivors (descending value, equal values in
    cell order).  A row whose k-th value is tied with a cell the partition left out is done by the definition.  +inf is a
    value that qualifies like any other (a total below 1 / DBL_MAX makes such rows)."""
    pp = np.asarray(postprob, np.float64)
    n, P = pp.shape
    if P <= k or n == 0:
        return select(pp, k, n_hla)
    with np.errstate(invalid="ignore"):
        c = np.where(pp > 0, pp, -np.inf)                    # zeros, negatives and NaN never qualify: -inf marks them
    cell = np.argpartition(-c, k - 1, axis=1)[:, :k]
    val = np.take_along_axis(c, cell, axis=1)
    order = np.lexsort((cell, -val), axis=1)
    cell, val = np.take_along_axis(cell, order, axis=1), np.take_along_axis(val, order, axis=1)
    thr = val[:, -1:]
    listed = val != -np.inf                                  # only the marker drops out: +inf is a value like any other
    cut = listed[:, -1] & ((c == thr).sum(axis=1) > (val == thr).sum(axis=1))               # a tie across the partition
    cell = np.where(listed, cell, -1)
    out = _finish(cell, np.where(listed, val, 0.0), k, n_hla)
    if cut.any():
        redo = select(pp[cut], k, n_hla)
        for key in KEYS:
            out[key][cut] = redo[key]
    return out


def topk(model, G, k: int, vote: int = 1, avx2: bool = True) -> dict:
    """The oracle's prediction of every sample of G (int32 [n_samp, n_snp]) and the selection from its posterior matrix:
    h1, h2, prob [n_samp, k], matching [n_samp]; ``call``: the oracle's own h1, h2, prob; ``postprob``: its matrix."""
    G = np.ascontiguousarray(G, np.int32)
    r = O.predict(O.flatten(model), G, vote_method=vote, want_dosage=False, want_prob=True, avx2=avx2,
                  n_threads=THREADS if avx2 else 1)
    out = select(r["postprob"], k, int(model.n_hla))
    out["matching"] = r["matching"]
    out["call"] = {"h1": r["h1"], "h2": r["h2"], "prob": r["prob"]}
    out["postprob"] = r["postprob"]
    return out


def assert_topk_equal(got, want, what="", keys=KEYS + ("matching",)):
    """Every entry of every key equal (NaN == NaN); the message names the first differing (sample, rank)."""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            continue
        bad = (a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a != b
        at = np.argwhere(bad)
        first = tuple(int(v) for v in at[0])
        raise AssertionError(f"{what} {key}: {len(at)} entries differ, the first at (sample, rank) {first}: "
                             f"got {a[first]!r}, reference {b[first]!r}")
