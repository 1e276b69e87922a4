#!/usr/bin/env python3
"""hlaAssocQuant at scale: one JSON line.

    python tools/assocquant_bench.py [--samples 10000] [--partitions 100] [--covariates 6] [--perms 10000] [--reps 3]

The cohort of tools/assoc_bench.py (HLA-B-sized allele list, 100 synthetic amino-acid partitions) with 6 standard-normal
covariates and a quantitative trait with a planted allele effect, the dominant model, 10,000 Freedman-Lane permutations:
end-to-end seconds of hlaAssocQuant (plan, device, host columns), of its device part alone (handles, observed run, all
permutations) and the event time of the FP64 Gram kernels within it, best of --reps, against a host baseline that does the
same analysis the way a user would in numpy on at most 16 threads -- QR of the covariates, ``Generator.permutation`` of the
residuals, and per 1,000 permutations one float64 matrix product features x residuals -- timed in the same run.  The two
sides are compared on the observed statistics (1e-9 relative) and, loosely, on the 95 % point of the distribution of the
maximum (two independent Monte-Carlo estimates: 5 %)."""

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
from hibag_amd import assoc, assocquant  # noqa: E402
from assoc_bench import cohort  # noqa: E402


def host_baseline(plan, y, covar, n_perm, seed):
    """(T_obs [device tests], max_stat [n_perm]) of the dominant model; NaN where the column is constant."""
    n = plan.n_samp
    table = np.concatenate([np.arange(len(plan.alleles))[None, :], plan.group_of])
    part = np.concatenate([np.zeros(len(plan.alleles), int)] + [np.full(int(g.max()) + 1, q + 1) for q, g in enumerate(plan.group_of)])
    lev = np.concatenate([np.arange(len(plan.alleles))] + [np.arange(int(g.max()) + 1) for g in plan.group_of])
    F = ((table[part][:, plan.a1] == lev[:, None]) | (table[part][:, plan.a2] == lev[:, None])).astype(np.float64)
    Q = np.linalg.qr(np.column_stack([np.ones(n), covar]))[0]              # [n, 1 + q]
    df = n - Q.shape[1] - 1
    P = F @ Q
    xx = (F * F).sum(axis=1)
    sxx = xx - (P * P).sum(axis=1)
    ok = (F.min(axis=1) != F.max(axis=1)) & (sxx > 1e-11 * xx)
    sxx = np.where(ok, sxx, np.nan)
    resid = y - Q @ (Q.T @ y)

    def stats(V):                                                           # V [k, n]: rows of (permuted) residuals
        R = V - (V @ Q) @ Q.T
        rr = (R * R).sum(axis=1)
        m = (F @ R.T) ** 2 / sxx[:, None]
        return m / ((rr[None, :] - m) / df)

    t_obs = stats(resid[None, :])[:, 0]
    rng = np.random.default_rng(seed)
    best = np.empty(n_perm)
    for p0 in range(0, n_perm, 1000):
        k = min(1000, n_perm - p0)
        V = np.stack([rng.permutation(resid) for _ in range(k)])
        best[p0:p0 + k] = np.nanmax(stats(V), axis=0)
    return t_obs, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--perms", type=int, default=10000)
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
    y = 10.0 + 0.25 * carrier + covar @ rng.uniform(-0.5, 0.5, a.covariates) + rng.standard_normal(a.samples)
    seed = 20240607

    hb.hlaAssocQuant(hla, y, covar, groups=groups, n_perm=64, seed=seed)       # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocQuant(hla, y, covar, model="dominant", groups=groups, n_perm=a.perms, seed=seed)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, np.zeros(a.samples, np.int32), float("nan"), groups)
    cov_t = np.ascontiguousarray(covar.T)
    dev_s, perm_s, gram_ms = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assocquant._DeviceQuant(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, 0) as dev:
            dev.quant(y, cov_t)
            t1 = time.perf_counter()
            dev.quant_permute(seed, 1, a.perms)
            perm_s.append(time.perf_counter() - t1)
            gram_ms.append(dev.quant_gram_ms())
        dev_s.append(time.perf_counter() - t0)

    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_obs, h_max = host_baseline(plan, y, covar, a.perms, seed)
        host_s.append(time.perf_counter() - t0)

    known = np.array(plan.row) >= 0
    d_obs = res.stat[known]
    both = np.isfinite(d_obs) & np.isfinite(h_obs)
    gap_obs = float(np.max(np.abs(d_obs / h_obs - 1)[both]))
    q_dev, q_host = float(np.quantile(res.max_stat, 0.95)), float(np.quantile(h_max, 0.95))
    close = bool(both.sum() >= 0.9 * len(h_obs) and np.array_equal(np.isfinite(d_obs), np.isfinite(h_obs)) and gap_obs <= 1e-9
                 and abs(q_dev / q_host - 1) <= 0.05)
    best, host = min(e2e), min(host_s)
    print(json.dumps({
        "tool": "assocquant_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "tests": len(res.name), "covariates": a.covariates, "model": "dominant", "perms": a.perms,
        "assoc_quant_s": round(best, 5), "assoc_quant_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "device_permute_s": round(min(perm_s), 5), "gram_ms": round(min(gram_ms), 4),
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / min(dev_s), 1),
        "compared": int(both.sum()), "observed_gap": gap_obs, "max95_device": round(q_dev, 4), "max95_host": round(q_host, 4),
        "top": res.name[int(np.nanargmax(res.stat))], "planted": planted,
        "top_perm_p_adj": float(res.perm_p_adj[int(np.nanargmax(res.stat))]), "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
