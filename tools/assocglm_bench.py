#!/usr/bin/env python3
"""hlaAssocGlm at scale: one JSON line.

    python tools/assocglm_bench.py [--samples 10000] [--partitions 100] [--covariates 6] [--reps 3]

The cohort of tools/assoc_bench.py (HLA-B-sized allele list, 100 synthetic amino-acid partitions) with 6 standard-normal
covariates that enter the phenotype, the dominant model: end-to-end seconds of hlaAssocGlm (plan, device, host columns) and
of its device part alone (handle, all fits), best of --reps, against a host baseline that does the same analysis the way a
user would in numpy -- per test a vectorised IRLS (the matrix products through BLAS on at most 16 threads, numpy.linalg
for the solve and the inverse, the same start value and stopping rule) -- timed in the same run.  The two sides are compared
on est and se of every test both fitted: 1e-6 in units of max(|est|, se) and 1e-6 relative (both stop at the same
criterion, so they differ by rounding and its amplification alone)."""

import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(int(os.environ.get(v, "16")), 16))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import assoc, assocglm  # noqa: E402
from assoc_bench import cohort  # noqa: E402


def host_fit(X, y, maxit=25, epsilon=1e-8):
    """(beta, se) of one logistic regression by IRLS, or None where it cannot be fitted."""
    mu = (y + 0.5) / 2.0
    eta = np.log(mu / (1 - mu))
    devold = np.inf
    for _ in range(maxit):
        mu = 1.0 / (1.0 + np.exp(-eta))
        W = mu * (1 - mu)
        z = eta + (y - mu) / W
        A = X.T @ (X * W[:, None])
        try:
            beta = np.linalg.solve(A, X.T @ (W * z))
        except np.linalg.LinAlgError:
            return None
        eta = X @ beta
        mu = np.clip(1.0 / (1.0 + np.exp(-eta)), 1e-300, 1 - 1e-16)
        dev = -2.0 * np.sum(np.where(y == 1, np.log(mu), np.log1p(-mu)))
        if abs(dev - devold) / (abs(dev) + 0.1) < epsilon:
            break
        devold = dev
    return beta, np.sqrt(np.diag(np.linalg.inv(A)))


def host_baseline(plan, covar):
    """est and se [device tests] of the h column, NaN where the column is constant."""
    n = plan.n_samp
    table = np.concatenate([np.arange(len(plan.alleles))[None, :], plan.group_of])
    part = np.concatenate([np.zeros(len(plan.alleles), int)] + [np.full(int(g.max()) + 1, q + 1) for q, g in enumerate(plan.group_of)])
    lev = np.concatenate([np.arange(len(plan.alleles))] + [np.arange(int(g.max()) + 1) for g in plan.group_of])
    F = ((table[part][:, plan.a1] == lev[:, None]) | (table[part][:, plan.a2] == lev[:, None])).astype(np.float64)
    y = plan.y.astype(np.float64)
    X = np.column_stack([np.ones(n), np.zeros(n), covar])
    est, se = np.full(len(F), np.nan), np.full(len(F), np.nan)
    for t, h in enumerate(F):
        if h.min() == h.max():
            continue
        X[:, 1] = h
        r = host_fit(X, y)
        if r is not None:
            est[t], se[t] = r[0][1], r[1][1]
    return est, se


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    hla, _, groups = cohort(a.samples, a.partitions)
    rng = np.random.default_rng(7)
    covar = rng.standard_normal((a.samples, a.covariates))
    names = hb.hlaUniqueAllele(list(hla.allele1) + list(hla.allele2))
    count = {k: 0 for k in names}
    for v in list(hla.allele1) + list(hla.allele2):
        count[v] += 1
    planted = sorted(names, key=lambda k: count[k])[-3]
    carrier = np.array([p == planted or q == planted for p, q in zip(hla.allele1, hla.allele2)])
    eta = -0.8 + 0.5 * carrier + covar @ (rng.uniform(-0.4, 0.4, a.covariates))
    y = (rng.random(a.samples) < 1 / (1 + np.exp(-eta))).astype(np.int32)

    hb.hlaAssocGlm(hla, y, covar, groups=groups)                       # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocGlm(hla, y, covar, model="dominant", groups=groups)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, y, float("nan"), groups)
    cov_t = np.ascontiguousarray(covar.T)
    dev_s, fit_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assocglm._DeviceGlm(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, 0) as dev:
            t1 = time.perf_counter()
            dev.glm(cov_t, None, 25, 1e-8)
            fit_s.append(time.perf_counter() - t1)
        dev_s.append(time.perf_counter() - t0)

    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_est, h_se = host_baseline(plan, covar)
        host_s.append(time.perf_counter() - t0)

    known = np.array(plan.row) >= 0
    d_est, d_se, d_fl = res.est[known, 0], res.se[known, 0], res.flags[known]
    both = (d_fl == 0) & np.isfinite(h_est)
    gap_est = float(np.max(np.abs(d_est - h_est)[both] / np.maximum(np.abs(h_est), h_se)[both]))
    gap_se = float(np.max(np.abs(d_se / h_se - 1)[both]))
    close = bool(both.sum() >= 0.9 * len(h_est) and gap_est <= 1e-6 and gap_se <= 1e-6)
    best, host = min(e2e), min(host_s)
    print(json.dumps({
        "tool": "assocglm_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "tests": len(res.name), "covariates": a.covariates, "model": "dominant",
        "assoc_glm_s": round(best, 5), "assoc_glm_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "device_fits_s": round(min(fit_s), 5),
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / min(dev_s), 1),
        "iterations_max": int(res.iterations.max()), "compared": int(both.sum()),
        "est_gap": gap_est, "se_gap": gap_se, "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
