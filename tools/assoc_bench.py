#!/usr/bin/env python3
"""hlaAssocTest with max-T permutation p-values at scale: one JSON line.

    python tools/assoc_bench.py [--samples 10000] [--partitions 100] [--perms 10000] [--reps 3]

A seeded synthetic cohort typed at the HLA-B-sized allele list of hibag_amd/synth.py, a case / control label enriched in the
carriers of one allele, 100 synthetic amino-acid partitions of the alleles (2 to 4 letters per position), the dominant model:
end-to-end seconds of hlaAssocTest (plan, device, host p-values) and of its device part alone (handle, observed statistics,
all permutations), against a host baseline that does the same analysis the way a user would -- labels from
numpy.random.Generator.permutation, one float32 matrix product per panel of permutations on at most 16 threads, a
vectorised Yates chi-square in float64, the running maximum and the counts -- timed in the same run.  The two sides draw
different permutations, so their p-values are compared loosely: the observed statistics to 1e-9, the 95 % point of the
maximum's distribution to 10 %."""

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
from hibag_amd import assoc, synth  # noqa: E402


def cohort(n_samp, n_part, seed=2025):
    model, _, freq = synth.make_model("hla-b", n_classifier=1, wide_classifier=False)
    alleles = list(model.hla_allele)
    rng = np.random.default_rng(seed)
    a = rng.choice(len(alleles), (n_samp, 2), p=freq)
    planted = int(np.argsort(freq)[-3])
    y = (rng.random(n_samp) < np.where((a == planted).any(axis=1), 0.42, 0.30)).astype(np.int32)
    hla = hb.hlaAllele([f"s{i}" for i in range(n_samp)], [alleles[i] for i in a[:, 0]], [alleles[i] for i in a[:, 1]], locus="B")
    letters = np.array(list("ARNDCQEG"))
    groups = None
    for q in range(n_part):
        lab = letters[rng.integers(0, rng.integers(2, 5), len(alleles))]
        one = hb.HlaAlleleGroups.from_labels(alleles, str(q + 1), list(lab))
        groups = one if groups is None else groups + one
    return hla, y, groups


def host_baseline(plan, n_perm, panel=1000, seed=1):
    """The same analysis on the host: (stat_obs, perm_p, perm_p_adj, max_stat)."""
    n, y = plan.n_samp, plan.y
    table = np.concatenate([np.arange(len(plan.alleles))[None, :], plan.group_of])
    part = np.concatenate([np.zeros(len(plan.alleles), int)] + [np.full(int(g.max()) + 1, q + 1) for q, g in enumerate(plan.group_of)])
    lev = np.concatenate([np.arange(len(plan.alleles))] + [np.arange(int(g.max()) + 1) for g in plan.group_of])
    F = ((table[part][:, plan.a1] == lev[:, None]) | (table[part][:, plan.a2] == lev[:, None])).astype(np.float32)
    r1 = F.sum(axis=1, dtype=np.float64)[:, None]
    c1 = float(y.sum())

    def chisq(x):
        det = n * x - r1 * c1
        d = np.maximum(2.0 * np.abs(det) - n, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return d * d * n / (4.0 * r1 * (n - r1) * c1 * (n - c1))

    obs = chisq((F @ y.astype(np.float32))[:, None].astype(np.float64))
    rng = np.random.default_rng(seed)
    count = np.zeros(len(F), np.int64)
    max_stat = np.empty(n_perm)
    yf = y.astype(np.float32)
    for p0 in range(0, n_perm, panel):
        k = min(panel, n_perm - p0)
        L = np.stack([rng.permutation(yf) for _ in range(k)])
        st = chisq((F @ L.T).astype(np.float64))
        with np.errstate(invalid="ignore"):
            count += (st >= obs).sum(axis=1)
        max_stat[p0:p0 + k] = np.nanmax(st, axis=0)
    with np.errstate(invalid="ignore"):
        count_max = (max_stat[None, :] >= obs).sum(axis=1)
    return obs[:, 0], (1 + count) / (n_perm + 1), (1 + count_max) / (n_perm + 1), max_stat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    hla, y, groups = cohort(a.samples, a.partitions)

    hb.hlaAssocTest(hla, y, groups=groups, n_perm=64, seed=1)               # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocTest(hla, y, model="dominant", groups=groups, n_perm=a.perms, seed=1)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, y, float("nan"), groups)
    dev_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assoc._DeviceAssoc(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, 0) as dev:
            dev.observed()
            dev.permute(1, 1, a.perms)
        dev_s.append(time.perf_counter() - t0)

    t0 = time.perf_counter()
    obs, _, adj, max_stat = host_baseline(plan, a.perms)
    t_host = time.perf_counter() - t0

    known = np.array(plan.row) >= 0
    d_obs = res.chisq_st[known]
    fin = ~np.isnan(obs)
    obs_close = bool(np.array_equal(np.isnan(d_obs), np.isnan(obs)) and np.allclose(d_obs[fin], obs[fin], rtol=1e-9, atol=1e-12))
    q_dev, q_host = float(np.quantile(res.max_stat, 0.95)), float(np.quantile(max_stat, 0.95))
    best = min(e2e)
    print(json.dumps({
        "tool": "assoc_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "tests": len(res.name), "perms": a.perms, "model": "dominant",
        "assoc_test_s": round(best, 5), "assoc_test_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "host_baseline_s": round(t_host, 4),
        "speedup_vs_host": round(t_host / best, 1), "device_part_speedup": round(t_host / min(dev_s), 1),
        "observed_close": obs_close, "max_stat_q95": [round(q_dev, 4), round(q_host, 4)],
        "smallest_adjusted_p": [float(np.nanmin(res.perm_p_adj)), float(np.nanmin(adj))],
    }))
    return 0 if obs_close and abs(q_dev - q_host) <= 0.1 * q_host else 1


if __name__ == "__main__":
    sys.exit(main())
