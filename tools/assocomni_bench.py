#!/usr/bin/env python3
"""hlaAssocOmnibus at scale: one JSON line.

    python tools/assocomni_bench.py [--samples 10000] [--partitions 100] [--covariates 6] [--reps 3]

An HLA-B-sized allele list, 100 synthetic amino-acid partitions of 2 to 8 levels, 6 standard-normal covariates that enter
the phenotype, one partition with a planted effect, the additive model: end-to-end seconds of hlaAssocOmnibus (plan, handle,
row sums, fits, host columns) and of its device part alone (handle, all fits), best of --reps, against a host baseline that
does the same analysis the way a user would in numpy -- per partition a vectorised IRLS on [1 | levels but the most frequent
| covariates] (the matrix products through BLAS on at most 16 threads, numpy.linalg for the solve, the same start value and
stopping rule) -- timed in the same run.  The two sides are compared on the deviance of every partition both fitted (1e-9
relative) and on the likelihood-ratio statistic (1e-6 absolute): both stop at the same criterion, so they differ by
rounding and its amplification alone."""

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
from hibag_amd import assoc, assocomni, synth  # noqa: E402


def cohort(n_samp, n_part, n_covar, seed=2026):
    """(hla, y, groups, covar [n, q]): partition 7's levels carry the planted effect."""
    model, _, freq = synth.make_model("hla-b", n_classifier=1, wide_classifier=False)
    alleles = list(model.hla_allele)
    rng = np.random.default_rng(seed)
    a = rng.choice(len(alleles), (n_samp, 2), p=freq)
    letters = np.array(list("ARNDCQEG"))
    labels = [rng.integers(0, rng.integers(2, 9), len(alleles)) for _ in range(n_part)]
    groups = None
    for q, lab in enumerate(labels):
        one = hb.HlaAlleleGroups.from_labels(alleles, str(q + 1), list(letters[lab]))
        groups = one if groups is None else groups + one
    covar = rng.standard_normal((n_samp, n_covar))
    planted = labels[min(7, n_part - 1)]
    effect = rng.uniform(-0.5, 0.5, 8)
    eta = -0.8 + effect[planted[a]].sum(axis=1) + covar @ rng.uniform(-0.4, 0.4, n_covar)
    y = (rng.random(n_samp) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    hla = hb.hlaAllele([f"s{i}" for i in range(n_samp)], [alleles[i] for i in a[:, 0]], [alleles[i] for i in a[:, 1]], locus="B")
    return hla, y, groups, covar


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
    """(deviance per partition, the base model's deviance): the dosage of every carried level but the most frequent."""
    n = plan.n_samp
    y = plan.y.astype(np.float64)
    ones = np.ones((n, 1))
    out = np.full(len(plan.group_of), np.nan)
    for p, g in enumerate(plan.group_of):
        k = int(g.max()) + 1
        D = (g[plan.a1][:, None] == np.arange(k)).astype(np.float64) + (g[plan.a2][:, None] == np.arange(k))
        s = D.sum(axis=0)
        carried = np.flatnonzero(s > 0)
        if len(carried) < 2:
            continue
        cols = [lv for lv in carried if lv != carried[np.argmax(s[carried])]]
        dev = host_fit(np.concatenate([ones, D[:, cols], covar], axis=1), y)
        if dev is not None:
            out[p] = dev
    return out, host_fit(np.concatenate([ones, covar], axis=1), y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    hla, y, groups, covar = cohort(a.samples, a.partitions, a.covariates)

    hb.hlaAssocOmnibus(hla, y, groups, covar)                          # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocOmnibus(hla, y, groups, covar)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, y, float("nan"), groups)
    cov_t = np.ascontiguousarray(covar.T)
    part_rows = assocomni._partition_rows(plan, groups)
    dev_s, fit_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assocomni._DeviceOmni(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, 1) as dev:
            sets = assocomni._design_sets(part_rows, dev.row_sums())[0]
            t1 = time.perf_counter()
            dev.glm_sets([[part_rows[p][lv] for lv in s] for p, s in enumerate(sets)], cov_t, None, 25, 1e-8)
            fit_s.append(time.perf_counter() - t1)
        dev_s.append(time.perf_counter() - t0)

    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_dev, h_base = host_baseline(plan, covar)
        host_s.append(time.perf_counter() - t0)

    both = (res.flags == 0) & np.isfinite(h_dev)
    gap_dev = float(np.max(np.abs(res.deviance / h_dev - 1)[both]))
    gap_lrt = float(np.max(np.abs(res.lrt_stat - (h_base - h_dev))[both]))
    close = bool(both.sum() >= 0.9 * len(h_dev) and gap_dev <= 1e-9 and gap_lrt <= 1e-6)
    best, host = min(e2e), min(host_s)
    top = int(np.nanargmin(res.lrt_p))
    print(json.dumps({
        "tool": "assocomni_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "covariates": a.covariates, "model": "additive", "columns_max": int(res.df.max()), "columns_total": int(res.df.sum()),
        "assoc_omnibus_s": round(best, 5), "assoc_omnibus_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "device_fits_s": round(min(fit_s), 5),
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / min(dev_s), 1),
        "iterations_max": int(res.iterations.max()), "compared": int(both.sum()), "top": res.name[top], "top_lrt_p": float(res.lrt_p[top]),
        "deviance_gap": gap_dev, "lrt_gap": gap_lrt, "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
