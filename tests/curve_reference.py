"""CPU reference of hlaPredictCurve for the tests: for each size the existing CPU oracle run on
``hlaSubModelObj(obj, size)``'s classifiers -- the reference's own hand loop (``hlaSubModelObj`` -> ``hlaModelFromObj`` ->
``hlaPredict``), built from the oracle alone.  ``first_classifiers`` restates the sub-model with ``dataclasses.replace`` so
that the yardstick does not depend on the function under test; tests/test_submodel_host.py pins the two equal."""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import oracle as O

KEYS = ("h1", "h2", "prob", "matching")
THREADS = 8


def first_classifiers(model, n: int):
    assert 1 <= n <= len(model.classifiers)
    return dataclasses.replace(model, classifiers=list(model.classifiers[:n]))


def curve(model, G, sizes=None, avx2: bool = True):
    """{h1, h2, prob, matching}, each [n_sizes, n_samp]: the oracle's prediction (vote by probability) of the model of
    the first sizes[i] classifiers."""
    sizes = list(range(1, len(model.classifiers) + 1)) if sizes is None else [int(s) for s in sizes]
    G = np.ascontiguousarray(G, np.int32)
    out = {"h1": np.empty((len(sizes), len(G)), np.int32), "h2": np.empty((len(sizes), len(G)), np.int32),
           "prob": np.empty((len(sizes), len(G))), "matching": np.empty((len(sizes), len(G)))}
    for i, k in enumerate(sizes):
        r = O.predict(O.flatten(first_classifiers(model, k)), G, vote_method=1, want_dosage=False, want_prob=False,
                      avx2=avx2, n_threads=THREADS if avx2 else 1)
        for key in KEYS:
            out[key][i] = r[key]
    return out


def same_bits(a, b) -> bool:
    """Equal values and NaN positions, and the same 64 bits wherever not NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a[keep].view(np.uint64), b[keep].view(np.uint64))


def assert_curve_equal(got, want, what=""):
    """Calls equal, prob and matching bit-equal, every size and sample; the message names the first differing (size row, sample)."""
    for key in KEYS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        ok = np.array_equal(a, b) if a.dtype.kind == "i" else same_bits(a, b)
        if ok:
            continue
        bad = a != b if a.dtype.kind == "i" else ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
        at = np.argwhere(bad)
        i, s = (int(v) for v in at[0])
        raise AssertionError(f"{what} {key}: {len(at)} entries differ, the first at size row {i}, sample {s} (group {s // 64}): "
                             f"got {a[i, s]!r}, reference {b[i, s]!r}")
