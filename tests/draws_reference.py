"""CPU reference of hlaPredictDraws for the tests: allele pairs drawn from the oracle's posterior matrix by the contract of
DESIGN.md section 16, restated in numpy.

``philox4x32_10`` is the generator (Salmon et al., SC'11), ``uniform(seed, index, t)`` the 53-bit uniform of draw ``t`` of
sample ``index``, ``draws_from_postprob`` the definition -- the sequential running sum of a sample's posterior in cell order
(``np.cumsum``; its last column is S, not ``np.sum``, which adds pairwise), the first cell with ``cum > u * S``, the last
positive cell should none qualify, NA for a sample whose ``S > 0`` is false -- and ``draws`` runs the oracle and draws."""

from __future__ import annotations

import numpy as np

from oracle import oracle as O
from topk_reference import pair_of_cell

NA_INTEGER = -2147483648
KEYS = ("h1", "h2", "prob")
THREADS = 8

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Ten rounds on counters [..., 4] and keys [..., 2] (anything that broadcasts; 32-bit values); returns uint32 [..., 4]."""
    c = np.asarray(counter, np.uint64) & _LO
    k = np.asarray(key, np.uint64) & _LO
    c0, c1, c2, c3 = (c[..., j] for j in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64: exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + np.uint64(W0)) & _LO, (k1 + np.uint64(W1)) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def uniform(seed, index, t):
    """u in [0, 1 - 2^-53] of draw ``t`` of sample ``index`` (arrays broadcast): ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = np.asarray(index, np.uint64)
    t = np.asarray(t, np.uint64)
    index, t = np.broadcast_arrays(index, t)
    counter = np.stack([index & _LO, index >> _32, t, np.zeros_like(t)], axis=-1)
    w = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).astype(np.uint64)
    return ((w[..., 0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[..., 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def draws_from_uniform(postprob: np.ndarray, u: np.ndarray, n_hla: int) -> dict:
    """The definition given the uniforms ``u`` [n_samp, n]: h1, h2 (int32) and prob, each [n_samp, n]."""
    pp = np.asarray(postprob, np.float64)
    assert pp.ndim == 2 and pp.shape[1] == n_hla * (n_hla + 1) // 2 and u.shape[0] == pp.shape[0]
    ns, P = pp.shape
    cum = np.cumsum(pp, axis=1)                        # sequential additions in cell order
    S = cum[:, -1]
    with np.errstate(invalid="ignore"):
        thr = u * S[:, None]                           # one multiply
        over = cum[:, None, :] > thr[:, :, None]       # [n_samp, n, n_cell]
        hit = over.any(axis=2)
        first = over.argmax(axis=2)
        pos = pp > 0
        last = np.where(pos.any(axis=1), P - 1 - pos[:, ::-1].argmax(axis=1), -1)
        ok = S > 0
    cell = np.where(hit, first, last[:, None])
    cell = np.where(ok[:, None], cell, -1)
    h1, h2 = pair_of_cell(cell, n_hla)
    prob = np.take_along_axis(pp, np.maximum(cell, 0), axis=1)
    none = np.where(np.isnan(S), np.nan, 0.0)
    prob = np.where(cell >= 0, prob, none[:, None])
    return {"h1": h1, "h2": h2, "prob": prob}


def draws_from_postprob(postprob: np.ndarray, n: int, seed: int, sample0: int, n_hla: int) -> dict:
    """The definition.  ``postprob`` [n_samp, n_cell] sample-major (the oracle's / ``predict_raw``'s); sample s of it is
    sample ``sample0 + s`` of the caller's numbering."""
    pp = np.asarray(postprob, np.float64)
    ns = pp.shape[0]
    u = uniform(seed, (np.arange(ns, dtype=np.uint64) + np.uint64(sample0))[:, None], np.arange(n, dtype=np.uint64)[None, :])
    u = u.reshape(ns, n)
    out = {key: np.empty((ns, n), np.float64 if key == "prob" else np.int32) for key in KEYS}
    step = max(1, (1 << 24) // max(1, n * pp.shape[1]))          # (bounds the [n_samp, n, n_cell] comparison)
    for a in range(0, ns, step):
        r = draws_from_uniform(pp[a:a + step], u[a:a + step], n_hla)
        for key in KEYS:
            out[key][a:a + step] = r[key]
    return out


def draws(model, G, n: int, seed: int, vote: int = 1, sample0: int = 0, avx2: bool = True) -> dict:
    """The oracle's prediction of every sample of G (int32 [n_samp, n_snp]) and the draws from its posterior matrix:
    h1, h2, prob [n_samp, n], matching [n_samp]; ``call``: the oracle's own h1, h2, prob; ``postprob``: its matrix."""
    G = np.ascontiguousarray(G, np.int32)
    r = O.predict(O.flatten(model), G, vote_method=vote, want_dosage=False, want_prob=True, avx2=avx2,
                  n_threads=THREADS if avx2 else 1)
    out = draws_from_postprob(r["postprob"], n, seed, sample0, int(model.n_hla))
    out["matching"] = r["matching"]
    out["call"] = {"h1": r["h1"], "h2": r["h2"], "prob": r["prob"]}
    out["postprob"] = r["postprob"]
    return out


def assert_draws_equal(got, want, what="", keys=KEYS + ("matching",)):
    """Every entry of every key equal (NaN == NaN); the message names the first differing (sample, draw)."""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            continue
        bad = (a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a != b
        at = np.argwhere(bad)
        first = tuple(int(v) for v in at[0])
        raise AssertionError(f"{what} {key}: {len(at)} entries differ, the first at (sample, draw) {first}: "
                             f"got {a[first]!r}, reference {b[first]!r}")
