"""The CPU oracle on whole synthetic cohorts, computed once and shared by the GPU tests that need it.

A kernel is only bit-exact if it is bit-exact on every sample: one wrong 64-sample group or one wrong chunk of a work item
passes any property check and most subsets.  So the tests at the benchmark's sizes compare every sample with the oracle's
AVX2 port (pinned equal to the scalar restatement: tests/test_oracle.py::test_avx2_threads_equal_scalar), and the results
are cached here per (shape, n, seed, missingness recipe, vote) so that tests sharing a cohort pay for it once.

Cohorts of more than SLICE samples are not cached whole (100,000 x 1,275 posterior cells are 1 GB per copy): compare
them with :func:`assert_same_sliced`, which runs the oracle one slice at a time."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

from hibag_amd import NA_INTEGER, synth
from oracle import oracle as O

KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")
THREADS = 8                       # (a fixed pool: the machines that run the suite have more cores than a job may use)
SLICE = 25_000


def _tail_one_step(model, count=10):
    """The last `count` classifiers of one K step.  Pass 1's work items are sorted by estimated work, stably; at the
    synthetic shapes every one-step classifier has as many haplotype pairs as the next, so the items that run last --
    the chunked rounds that resume at HibagModelView::blk_close rows -- are those of the highest indices."""
    return [c for c, cls in enumerate(model.classifiers) if len(cls.snpidx) <= 32][-count:]


def _structured(model, G):
    """One 64-sample group near the end that misses every SNP of the ten classifiers of the chunked tail; groups that miss
    a third, or all but one, of some classifiers' SNPs (weights that are not powers of two: 2/3, 1/k); an all-NA last
    sample."""
    n = G.shape[0]
    snps = [np.asarray(c.snpidx) for c in model.classifiers]
    tail = _tail_one_step(model)
    g = n // 64 - 3
    for c in tail:
        G[np.ix_(range(64 * g, 64 * g + 64), snps[c])] = NA_INTEGER
    for c in tail[::2] + [0, 1, 2]:
        G[np.ix_(range(64 * (g + 1), 64 * (g + 1) + 50), snps[c][::3])] = NA_INTEGER
        G[np.ix_(range(64 * (g - 1) + 10, 64 * g), snps[c][1:])] = NA_INTEGER
    G[n - 1, :] = NA_INTEGER


RECIPES = {
    "": lambda model, G: None,
    "na5": lambda model, G: G.__setitem__((5, slice(None)), NA_INTEGER),
    "na7": lambda model, G: G.__setitem__((7, slice(None)), NA_INTEGER),
    "structured": _structured,
}


@functools.lru_cache(maxsize=8)
def cohort(shape: str, n: int, seed: int = synth.DEFAULT_SEED + 1, recipe: str = ""):
    """(model, G, truth) of synth.make_model(shape) and n samples of synth.make_samples(seed), `recipe` applied.
    G is read-only: a test that changes it must copy it (and then cannot use the cached oracle results)."""
    model, founders, af = synth.make_model(shape)
    G, truth = synth.make_samples(founders, af, n, seed=seed)
    RECIPES[recipe](model, G)
    G.setflags(write=False)
    return model, G, truth


@functools.lru_cache(maxsize=8)
def _flat(shape: str):
    return O.flatten(synth.make_model(shape)[0])


@functools.lru_cache(maxsize=6)
def want(shape: str, n: int, vote: int = 1, seed: int = synth.DEFAULT_SEED + 1, recipe: str = "", want_prob: bool = True):
    """The oracle's outputs for every sample of cohort(shape, n, seed, recipe)."""
    if n > SLICE:
        raise ValueError(f"{n} samples: compare in slices (assert_same_sliced)")
    _, G, _ = cohort(shape, n, seed, recipe)
    out = O.predict(_flat(shape), G, vote_method=vote, want_prob=want_prob, avx2=True, n_threads=THREADS)
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_same(got, ref, keys=KEYS, offset=0, what=""):
    """Every entry of every key bit-equal (NaN == NaN); the message names the first differing sample and its 64-sample
    group.  `offset`: index of ref's first sample in the cohort (for the message)."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if np.array_equal(a, b, equal_nan=True):
            continue
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a != b
        rows = np.flatnonzero(bad.reshape(len(a), -1).any(axis=1))
        s = int(rows[0])
        raise AssertionError(f"{what} {k}: {len(rows)} samples differ, the first is sample {offset + s} (group "
                             f"{(offset + s) // 64}): got {a[s]!r}, oracle {b[s]!r}; groups "
                             f"{sorted(set(((offset + rows) // 64).tolist()))[:20]}")


def assert_same_sliced(got, model, G, vote=1, keys=KEYS, step=SLICE):
    """`got` (outputs for every sample of G) against the oracle, SLICE samples at a time."""
    fm = O.flatten(model)
    want_prob = "postprob" in keys
    for lo in range(0, G.shape[0], step):
        ref = O.predict(fm, G[lo:lo + step], vote_method=vote, want_prob=want_prob, avx2=True, n_threads=THREADS)
        assert_same({k: got[k][lo:lo + step] for k in keys}, ref, keys, offset=lo, what=f"vote {vote}")


# ---- hlaOutOfBag: the reference's per-classifier loop on the oracle --------------------------------------------------

def bootstrap(n_classifier: int, n: int, seed: int) -> np.ndarray:
    """Seeded bootstrap counts [n_classifier, n]: n draws with replacement per classifier (about 37 % out of bag)."""
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(n_classifier)]).astype(np.int32)


def oob_loop(model, G, samp_num, avx2=True):
    """Classifier by classifier, a one-classifier model predicts its out-of-bag samples (vote "prob"): [C, n] arrays."""
    from test_oob_host import oracle_oob
    m = dataclasses.replace(model, classifiers=[dataclasses.replace(c, samp_num=s) for c, s in zip(model.classifiers, samp_num)])
    return oracle_oob(O, m, G, avx2=avx2, n_threads=THREADS if avx2 else 1)


@functools.lru_cache(maxsize=2)
def want_oob(shape: str, n: int, boot_seed: int, seed: int = synth.DEFAULT_SEED + 1, recipe: str = ""):
    model, G, _ = cohort(shape, n, seed, recipe)
    sn = bootstrap(len(model.classifiers), n, boot_seed)
    sn.setflags(write=False)
    return sn, oob_loop(model, G, sn)
