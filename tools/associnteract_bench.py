#!/usr/bin/env python3
"""hlaAssocInteract at scale: one JSON line.

    python tools/associnteract_bench.py [--samples 10000] [--covariates 6] [--reps 3]

An HLA-B-sized allele list of 50 (49 of them carried at the default size), 6 standard-normal covariates that enter the phenotype, one planted interaction of two
alleles, the additive model, all carried pairs: end-to-end seconds of hlaAssocInteract (plan, handle, row sums, the Gram
of the feature rows, two fits per pair, host columns) and of its device part alone (handle, Gram, all fits), best of --reps,
against a host baseline that does the same scan the way a user would in numpy -- per fit a vectorised IRLS on
[1 | a | b | (a b) | covariates] (the matrix products through BLAS on at most 16 threads, numpy.linalg for the solve, the same
start value and stopping rule) -- timed in the same run.  The two sides are compared on both deviances of every pair both
fitted without a flag (1e-9 relative) and on the likelihood-ratio statistic (1e-6 absolute): both stop at the same
criterion, so they differ by rounding and its amplification alone."""

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
from hibag_amd import assoc, associnteract, synth  # noqa: E402


def cohort(n_samp, n_covar, seed=2027):
    """(hla, y, covar [n, q], the planted pair's names): the two most frequent alleles interact."""
    model, _, freq = synth.make_model("hla-b", n_classifier=1, wide_classifier=False)
    alleles = list(model.hla_allele)
    rng = np.random.default_rng(seed)
    a = rng.choice(len(alleles), (n_samp, 2), p=freq)
    top = np.argsort(-np.asarray(freq), kind="stable")[:2]
    d = [(a == k).sum(axis=1) for k in top]
    covar = rng.standard_normal((n_samp, n_covar))
    eta = -0.8 + 0.2 * d[0] - 0.2 * d[1] + 1.2 * d[0] * d[1] + covar @ rng.uniform(-0.4, 0.4, n_covar)
    y = (rng.random(n_samp) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    hla = hb.hlaAllele([f"s{i}" for i in range(n_samp)], [alleles[i] for i in a[:, 0]], [alleles[i] for i in a[:, 1]], locus="B")
    return hla, y, covar, sorted(alleles[k] for k in top)


def host_fit(X, y, maxit=25, epsilon=1e-8):
    """The deviance of one logistic regression by IRLS, or None where it cannot be fitted."""
    mu = (y + 0.5) / 2.0
    eta = np.log(mu / (1 - mu))
    devold = np.inf
    dev = np.nan
    for _ in range(maxit):
        mu = 1.0 / (1.0 + np.exp(-eta))
        W = mu * (1 - mu)
        z = eta + (y - mu) / W
        try:
            beta = np.linalg.solve(X.T @ (X * W[:, None]), X.T @ (W * z))
        except np.linalg.LinAlgError:
            return None
        eta = X @ beta
        mu = np.clip(1.0 / (1.0 + np.exp(-eta)), 1e-300, 1 - 1e-16)
        dev = -2.0 * np.sum(np.where(y == 1, np.log(mu), np.log1p(-mu)))
        if abs(dev - devold) / (abs(dev) + 0.1) < epsilon:
            break
        devold = dev
    return dev


def host_baseline(plan, covar):
    """(deviance of the main fit, of the full fit) per pair of carried alleles with a carrier of both, in the scan's order."""
    n, k = plan.n_samp, len(plan.alleles)
    y = plan.y.astype(np.float64)
    D = (plan.a1[:, None] == np.arange(k)).astype(np.float64) + (plan.a2[:, None] == np.arange(k))
    ones = np.ones((n, 1))
    both = D.T @ D
    main, full = [], []
    for a in range(k):
        for b in range(a + 1, k):
            if both[a, b] < 1:
                main.append(np.nan)
                full.append(np.nan)
                continue
            X = np.concatenate([ones, D[:, [a, b]], covar], axis=1)
            m = host_fit(X, y)
            f = host_fit(np.concatenate([X, (D[:, a] * D[:, b])[:, None]], axis=1), y)
            main.append(np.nan if m is None else m)
            full.append(np.nan if f is None else f)
    return np.array(main), np.array(full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    hla, y, covar, planted = cohort(a.samples, a.covariates)

    hb.hlaAssocInteract(hla, y, covar)                                 # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocInteract(hla, y, covar)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, y, float("nan"), None)
    cov_t = np.ascontiguousarray(covar.T)
    dev_s, fit_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with associnteract._DeviceInteract(plan.a1, plan.a2, plan.y, len(plan.alleles), None, 1) as dev:
            rows, _, _ = associnteract._pair_rows(plan, None, dev.row_sums())
            both = associnteract._both(dev, rows)
            terms = np.array([t for (r, s), c in zip(rows, both) if c >= 1
                              for t in ([(r, -1), (s, -1), (-1, -1)], [(r, -1), (s, -1), (r, s)])], np.int32)
            t1 = time.perf_counter()
            dev.glm_terms(terms, cov_t, None, 25, 1e-8)
            fit_s.append(time.perf_counter() - t1)
        dev_s.append(time.perf_counter() - t0)

    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_main, h_full = host_baseline(plan, covar)
        host_s.append(time.perf_counter() - t0)

    ok = (res.flags_main == 0) & (res.flags_full == 0) & np.isfinite(h_main) & np.isfinite(h_full)
    gap_dev = float(max(np.max(np.abs(res.deviance_main / h_main - 1)[ok]), np.max(np.abs(res.deviance_full / h_full - 1)[ok])))
    gap_lrt = float(np.max(np.abs(res.lrt_stat - (h_main - h_full))[ok]))
    fitted = int(((res.flags_full & 2) == 0).sum())
    close = bool(len(h_main) == len(res.both) and ok.sum() >= 0.5 * fitted and gap_dev <= 1e-9 and gap_lrt <= 1e-6)
    best, host = min(e2e), min(host_s)
    top = int(np.nanargmin(res.lrt_p))
    print(json.dumps({
        "tool": "associnteract_bench", "samples": a.samples, "alleles": len(plan.alleles), "pairs": len(res.both),
        "pairs_fitted": fitted, "fits": 2 * fitted + 1, "covariates": a.covariates, "model": "additive",
        "assoc_interact_s": round(best, 5), "assoc_interact_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "device_fits_s": round(min(fit_s), 5),
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / min(dev_s), 1),
        "iterations_max": int(max(res.iterations_main.max(), res.iterations_full.max())), "compared": int(ok.sum()),
        "top": [res.name_a[top], res.name_b[top]], "planted": planted, "top_lrt_p": float(res.lrt_p[top]),
        "deviance_gap": gap_dev, "lrt_gap": gap_lrt, "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
