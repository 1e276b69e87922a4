#!/usr/bin/env python3
"""hlaHaplotypes at scale: one JSON line.

    python tools/haplo_bench.py [--samples 10000] [--loci 4] [--k 3] [--pool 40] [--alleles 30] [--reps 3] [--host-reps 1]

A synthetic cohort with linkage disequilibrium: every chromosome is drawn from a pool of --pool haplotypes over --loci loci
with Dirichlet frequencies; per sample and locus the true pair and k - 1 decoys that share one allele with it, with
probabilities from a Dirichlet draw, and in 30 % of the lists the true pair demoted to rank 1 behind a decoy.  Timed, best of
--reps: hlaHaplotypes end to end (gather, trimming, device, result), and its device parts alone (the handle: states, sort,
dictionary, work lists; the fit; the calls).  The host baseline is a vectorised numpy EM of the same model on at most 16
threads -- states enumerated with array operations over the (candidate, phase) grid, np.unique for the dictionary, np.bincount
for the E step's totals and the M step -- timed in the same run (--host-reps times), enumeration and iterations apart.  The two sides share the
model but not the order of their sums, so they are compared with a tolerance: the frequencies to 10 tol (a stop one iteration
apart moves them by about tol), the iteration counts to +- 1, the calls of the samples whose best posterior leads by more than 1e-6."""

import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(int(os.environ.get(v, "16")), 16))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import haplo  # noqa: E402
from hibag_amd.topk import HlaTopCalls  # noqa: E402


def cohort(n, L, k, n_pool, n_allele, seed):
    """(truth lo, hi [L, n]; h1, h2, prob [L, n, k])."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, n_allele, size=(n_pool, L))
    w = rng.dirichlet(np.full(n_pool, 0.5))
    a, b = pool[rng.choice(n_pool, n, p=w)].T, pool[rng.choice(n_pool, n, p=w)].T
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    x = np.stack([lo] * k, axis=2)
    y = np.stack([(hi + r) % n_allele for r in range(k)], axis=2)             # rank 0: the truth; decoys keep `lo`
    p = -np.sort(-rng.dirichlet(np.full(k, 2.0), size=(L, n)), axis=2)
    if k > 1:
        swap = rng.random((L, n)) < 0.3
        y[swap, 0], y[swap, 1] = y[swap, 1], y[swap, 0].copy()
    return (lo, hi), np.minimum(x, y).astype(np.int32), np.maximum(x, y).astype(np.int32), p


def host_states(h1, h2, prob):
    """The states of every sample by array operations: (wc, key A, key B, sample) of the valid cells of the grid
    [n, k^L combinations, 2^(L - 1) phase masks]."""
    L, n, k = h1.shape
    ranks = np.indices((k,) * L).reshape(L, -1)                       # [L, C]: locus L - 1 fastest
    a1 = np.stack([h1[l][:, ranks[l]] for l in range(L)]).astype(np.int64)   # [L, n, C]
    a2 = np.stack([h2[l][:, ranks[l]] for l in range(L)]).astype(np.int64)
    w = prob[0][:, ranks[0]]
    for l in range(1, L):
        w = w * prob[l][:, ranks[l]]
    het = a1 != a2
    n_het = het.sum(axis=0)
    bit = np.cumsum(het, axis=0) - het - 1                            # the phase bit of a heterozygous locus; -1: the anchor
    slots = 1 << np.maximum(n_het - 1, 0)
    wc = w * np.where(n_het > 0, 2.0, 1.0)
    out = []
    for m in range(1 << (L - 1)):
        ok = (m < slots) & (w > 0)
        swap = het & (bit >= 0) & (((m >> np.maximum(bit, 0)) & 1) == 1)
        ka = sum(np.where(swap[l], a2[l], a1[l]) << (10 * l) for l in range(L))
        kb = sum(np.where(swap[l], a1[l], a2[l]) << (10 * l) for l in range(L))
        s = np.broadcast_to(np.arange(n)[:, None], ok.shape)
        c = np.broadcast_to(np.arange(ok.shape[1])[None, :], ok.shape)
        out.append((wc[ok], ka[ok], kb[ok], s[ok], c[ok] * (1 << (L - 1)) + m))
    wc, ka, kb, s, order = (np.concatenate(v) for v in zip(*out))
    at = np.lexsort((order, s))                                       # state order: sample, combination, mask
    return wc[at], ka[at], kb[at], s[at]


def host_em(wc, ka, kb, samp, n, maxit, tol):
    keys, inv = np.unique(np.concatenate([ka, kb]), return_inverse=True)
    iA, iB = inv[:len(ka)], inv[len(ka):]
    H = len(keys)
    f = np.full(H, 1.0 / H)
    for it in range(1, maxit + 1):
        g = wc * f[iA] * f[iB]
        tot = np.bincount(samp, g, n)
        q = g / tot[samp]
        fn = (np.bincount(iA, q, H) + np.bincount(iB, q, H)) / (2.0 * n)
        delta = float(np.abs(fn - f).max())
        f = fn
        if delta <= tol:
            break
    g = wc * f[iA] * f[iB]
    q = g / np.bincount(samp, g, n)[samp]
    return keys, f, it, delta, q, iA, iB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--loci", type=int, default=4)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--pool", type=int, default=40)
    ap.add_argument("--alleles", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-8)
    a = ap.parse_args()
    n, L, k = a.samples, a.loci, a.k
    truth, h1, h2, prob = cohort(n, L, k, a.pool, a.alleles, 1)
    ids = [f"s{i}" for i in range(n)]
    calls = {f"L{l}": HlaTopCalls(f"L{l}", ids, k, h1[l], h2[l], prob[l], np.ones(n), levels=[f"L{l}*{i:02d}" for i in range(a.alleles)])
             for l in range(L)}
    kw = dict(min_prob=0.0, maxit=200, tol=a.tol, verbose=False)

    hb.hlaHaplotypes(calls, **kw)                                     # warm-up: code objects, allocations
    e2e, new_s, fit_s, call_s = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaHaplotypes(calls, **kw)
        e2e.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        with haplo._DeviceHaplo(h1, h2, prob, 4096) as dev:
            t1 = time.perf_counter()
            dev.fit(200, a.tol)
            t2 = time.perf_counter()
            dev.calls()
            t3 = time.perf_counter()
        new_s.append(t1 - t0); fit_s.append(t2 - t1); call_s.append(t3 - t2)

    enum_s, em_s = [], []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        wc, ka, kb, samp = host_states(h1, h2, prob)
        t1 = time.perf_counter()
        keys, f, it, delta, q, iA, iB = host_em(wc, ka, kb, samp, n, 200, a.tol)
        t2 = time.perf_counter()
        enum_s.append(t1 - t0); em_s.append(t2 - t1)

    # the comparison
    order = np.argsort(res.keys)
    assert np.array_equal(res.keys[order], keys.astype(np.uint64)), "the two sides disagree on the dictionary"
    assert len(wc) == int(res.n_states.sum()), "the two sides disagree on the states"
    freq_diff = float(np.abs(res.freq[order] - f).max())
    assert freq_diff <= 10 * a.tol, freq_diff
    assert abs(res.n_iter - it) <= 1, (res.n_iter, it)
    first = np.concatenate([[0], np.cumsum(res.n_states)[:-1]])
    best = np.array([s0 + int(np.argmax(q[s0:s0 + c])) for s0, c in zip(first, res.n_states)])
    lead = np.array([np.partition(q[s0:s0 + c], -2)[-2:] if c > 1 else [0.0, 1.0] for s0, c in zip(first, res.n_states)])
    clear = (lead[:, 1] - lead[:, 0]) > 1e-6
    same = (haplo.decode_keys(keys[iA[best]], L) == res.h1).all(axis=1) & (haplo.decode_keys(keys[iB[best]], L) == res.h2).all(axis=1)
    assert same[clear].all(), "the two sides disagree on a clear call"
    lo, hi = np.minimum(res.h1, res.h2).T, np.maximum(res.h1, res.h2).T
    before = int(((h1[:, :, 0] == truth[0]) & (h2[:, :, 0] == truth[1])).sum())
    after = int(((lo == truth[0]) & (hi == truth[1])).sum())
    host = min(x + y for x, y in zip(enum_s, em_s))
    print(json.dumps({
        "samples": n, "loci": L, "k": k, "states": int(res.n_states.sum()), "haplotypes": len(res.freq), "iterations": res.n_iter,
        "host_iterations": it, "delta": res.delta, "converged": res.converged, "max_freq_diff": freq_diff,
        "calls_compared": int(clear.sum()), "correct_pairs_rank0": before, "correct_pairs_joint": after, "pairs": n * L,
        "e2e_s": round(min(e2e), 5), "e2e_s_all": [round(x, 5) for x in e2e], "handle_s": round(min(new_s), 5),
        "fit_s": round(min(fit_s), 5), "fit_ms_per_iteration": round(1e3 * min(fit_s) / res.n_iter, 4), "calls_s": round(min(call_s), 5),
        "host_s": round(host, 5), "host_enumerate_s": round(min(enum_s), 5), "host_em_s": round(min(em_s), 5),
        "host_em_ms_per_iteration": round(1e3 * min(em_s) / it, 3), "host_threads": int(os.environ["OMP_NUM_THREADS"]),
        "speedup_e2e": round(host / min(e2e), 2), "speedup_em": round(min(em_s) / min(fit_s), 2)}))


if __name__ == "__main__":
    main()
