"""CPU reference of a per-sample classifier mask (``HlaAttrBagClass.predict_masked``, ``hlaOutOfBagEnsemble``) for the
tests, built from the oracle alone: sample s gets what the oracle predicts for it from the model made of the classifiers
c with ``use[c, s] != 0``, in model order -- the hand loop (sub-model -> ``hlaModelFromObj`` -> ``hlaPredict``) restated
with ``dataclasses.replace``.  Samples that share a mask column share a sub-model, so they are predicted together; a sample
no classifier is used for gets what the full model returns for a sample with every SNP missing."""

from __future__ import annotations

import dataclasses

import numpy as np

from hibag_amd import NA_INTEGER
from oracle import oracle as O

KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")
THREADS = 8


def kept(model, column):
    return dataclasses.replace(model, classifiers=[c for c, u in zip(model.classifiers, column) if u])


def masked(model, G, use, vote_method: int = 1, avx2: bool = True):
    """{h1, h2, prob, matching [n_samp], dosage [n_samp, n_hla], postprob [n_samp, n_cell]} for ``use`` [n_classifier, n_samp]."""
    G = np.ascontiguousarray(G, np.int32)
    use = np.asarray(use) != 0
    n = len(G)
    assert use.shape == (len(model.classifiers), n)
    P = model.n_hla * (model.n_hla + 1) // 2
    out = {"h1": np.empty(n, np.int32), "h2": np.empty(n, np.int32), "prob": np.empty(n), "matching": np.empty(n),
           "dosage": np.empty((n, model.n_hla)), "postprob": np.empty((n, P))}
    groups = {}
    for s in range(n):
        groups.setdefault(use[:, s].tobytes(), []).append(s)
    full = None
    for key, rows in groups.items():
        column = np.frombuffer(key, bool)
        if column.any():
            r = O.predict(O.flatten(kept(model, column)), G[rows], vote_method, want_dosage=True, want_prob=True,
                          avx2=avx2, n_threads=THREADS if avx2 else 1)
        else:
            if full is None:
                full = O.predict(O.flatten(model), np.full((1, G.shape[1]), NA_INTEGER, np.int32), vote_method,
                                 want_dosage=True, want_prob=True)
            r = {k: np.repeat(full[k], len(rows), axis=0) for k in KEYS}
        for k in KEYS:
            out[k][rows] = r[k]
    return out


def same_bits(got, want, what="", keys=KEYS):
    """Calls equal and every float the same 64 bits (NaN against NaN counts as equal); the message names the first
    differing (field, sample, 64-sample group)."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if a.dtype.kind == "i":
            bad = a != b
        else:
            a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
            bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
        if bad.any():
            at = np.argwhere(bad)
            s = int(at[0][0])
            raise AssertionError(f"{what} {k}: {len(at)} entries differ, the first at sample {s} (group {s // 64})"
                                 f"{'' if a.ndim == 1 else f', column {int(at[0][1])}'}: got {a[tuple(at[0])]!r}, "
                                 f"reference {b[tuple(at[0])]!r}")
    return True


def bootstrap(n_classifier: int, n: int, seed: int) -> np.ndarray:
    """Seeded bootstrap counts [n_classifier, n]: ``bincount`` of n draws per classifier."""
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, n, n), minlength=n).astype(np.int32) for _ in range(n_classifier)])
