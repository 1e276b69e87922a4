#!/usr/bin/env python3
"""hlaAssocScore at scale: one JSON line.

    python tools/assocscore_bench.py [--samples 10000] [--partitions 100] [--covariates 6] [--perms 10000] [--reps 3]

The cohort of tools/assoc_bench.py (HLA-B-sized allele list, 100 synthetic amino-acid partitions, a case / control label with
a planted allele effect) with 6 standard-normal covariates, the dominant model, 10,000 sign replicates: end-to-end seconds of
hlaAssocScore (plan, base fit, device, host columns), of its device part alone (handles, base fit, sets, observed run, all
replicates), the event times of the resampling call split into residual panels (signs, projection, panel write), FP64 Gram
and statistics, and the host's min-P step, best of --reps; the same for the omnibus form over the partitions.  The host
baseline does the same analysis the way a user would in numpy on at most 16 threads -- IRLS for the base model, QR of the
weighted covariates, an explicit sign matrix and per 1,000 replicates one float64 matrix product features x residuals --
timed in the same run.  The two sides are compared on the observed statistics (1e-9 relative; the omnibus form on its
observed statistics too) and on the 5 % point of the replicates' smallest p-value within its sampling error: two independent
Monte-Carlo estimates of a 5 % quantile from N replicates each differ by 4 standard errors at most,
4 sqrt(2 x 0.05 x 0.95 / N) / 0.05 relative (0.25 at N = 10,000)."""

import argparse
import json
import math
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
from hibag_amd import assoc, assocomni, assocscore  # noqa: E402
from assoc_bench import cohort  # noqa: E402


def features(plan, additive=False):
    table = np.concatenate([np.arange(len(plan.alleles))[None, :], plan.group_of])
    part = np.concatenate([np.zeros(len(plan.alleles), int)] + [np.full(int(g.max()) + 1, q + 1) for q, g in enumerate(plan.group_of)])
    lev = np.concatenate([np.arange(len(plan.alleles))] + [np.arange(int(g.max()) + 1) for g in plan.group_of])
    d = (table[part][:, plan.a1] == lev[:, None]).astype(np.float64) + (table[part][:, plan.a2] == lev[:, None])
    return d if additive else (d >= 1).astype(np.float64)


def base_model(y, covar):
    """(w, e, Qw): IRLS of y ~ 1 + covar, the weights mu (1 - mu), the residuals, and the orthonormal basis of sqrt(w) Z."""
    Z = np.column_stack([np.ones(len(y)), covar])
    beta = np.zeros(Z.shape[1])
    for _ in range(25):
        mu = 1.0 / (1.0 + np.exp(-(Z @ beta)))
        w = mu * (1.0 - mu)
        step = np.linalg.solve(Z.T @ (Z * w[:, None]), Z.T @ (y - mu))
        beta += step
        if np.abs(step).max() < 1e-12:
            break
    mu = 1.0 / (1.0 + np.exp(-(Z @ beta)))
    w = mu * (1.0 - mu)
    return w, y - mu, np.linalg.qr(Z * np.sqrt(w)[:, None])[0]


def host_baseline(F, y, covar, n_perm, seed):
    """(T_obs [rows], min_p [n_perm]) of one-column score tests; NaN where the column is constant."""
    w, e, Qw = base_model(y, covar)
    sw = np.sqrt(w)
    Xw = F * sw                                                              # [rows, n]
    Xt = (Xw - (Xw @ Qw) @ Qw.T) / sw                                        # x~ = x - Q (Q' W x)
    V = (Xt * Xt * w).sum(axis=1)
    ok = (F.min(axis=1) != F.max(axis=1)) & (V > 1e-11 * (F * F * w).sum(axis=1))
    V = np.where(ok, V, np.nan)
    t_obs = (Xt @ e) ** 2 / V
    rng = np.random.default_rng(seed)
    best = np.empty(n_perm)
    for p0 in range(0, n_perm, 1000):
        k = min(1000, n_perm - p0)
        s = rng.integers(0, 2, (k, len(y))).astype(np.float64) * 2.0 - 1.0
        best[p0:p0 + k] = np.nanmax((Xt @ (s * e).T) ** 2 / V[:, None], axis=0)
    return t_obs, np.array([math.erfc(math.sqrt(t / 2.0)) for t in best])


def host_omnibus(F, sets, y, covar):
    """U' V^-1 U of every set of rows with at least one row, by numpy.linalg.solve."""
    w, e, Qw = base_model(y, covar)
    sw = np.sqrt(w)
    out = np.full(len(sets), np.nan)
    for t, rows in enumerate(sets):
        if rows:
            Xw = F[rows] * sw
            Xt = (Xw - (Xw @ Qw) @ Qw.T) / sw
            U = Xt @ e
            out[t] = U @ np.linalg.solve((Xt * w) @ Xt.T, U)
    return out


def timed(hla, y, covar, groups, plan, model, omnibus, perms, reps, seed):
    """Best-of-reps times of one form: (result, dict of seconds and milliseconds)."""
    hb.hlaAssocScore(hla, y, covar, model, groups=groups, omnibus=omnibus, n_perm=64, seed=seed)       # warm-up: code objects, allocations
    e2e = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocScore(hla, y, covar, model, groups=groups, omnibus=omnibus, n_perm=perms, seed=seed)
        e2e.append(time.perf_counter() - t0)
    cov_t = np.ascontiguousarray(covar.T)
    dev_s, res_s, ms = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with assocscore._DeviceScore(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, assoc.MODELS.index(model)) as dev:
            rsum = dev.row_sums()
            if omnibus:
                part_rows = assocomni._partition_rows(plan, groups)
                sets = [[part_rows[p][lv] for lv in s] for p, s in enumerate(assocomni._design_sets(part_rows, rsum)[0])]
            else:
                sets = assocscore._single_sets(model, rsum, plan.n_samp)
            dev.score(cov_t, None, 25, 1e-8)
            dev.score_sets(sets)
            t1 = time.perf_counter()
            max_stat, _ = dev.score_resample(seed, 1, perms)
            res_s.append(time.perf_counter() - t1)
            ms.append(dev.score_ms())
        dev_s.append(time.perf_counter() - t0)
    minp_s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assocscore._min_p(res.max_stat, res.max_stat_df.tolist())
        minp_s.append(time.perf_counter() - t0)
    k = int(np.argmin([sum(m) for m in ms]))
    return res, sets, {"e2e_s": round(min(e2e), 5), "e2e_s_all": [round(x, 5) for x in e2e], "device_part_s": round(min(dev_s), 5),
                       "resample_call_s": round(min(res_s), 5), "project_ms": round(ms[k][0], 3), "gram_ms": round(ms[k][1], 3),
                       "stat_ms": round(ms[k][2], 3), "host_min_p_s": round(min(minp_s), 5), "df_values": res.max_stat_df.tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--partitions", type=int, default=100)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    hla, y, groups = cohort(a.samples, a.partitions)
    covar = np.random.default_rng(7).standard_normal((a.samples, a.covariates))
    seed = 20240607
    plan = assoc._Plan(hla, y, float("nan"), groups)

    res, _, single = timed(hla, y, covar, groups, plan, "dominant", False, a.perms, a.reps, seed)
    omni, omni_sets, omnibus = timed(hla, y, covar, groups, plan, "additive", True, a.perms, a.reps, seed)

    F = features(plan)
    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_obs, h_minp = host_baseline(F, plan.y.astype(np.float64), covar, a.perms, seed)
        host_s.append(time.perf_counter() - t0)
    known = np.array(plan.row) >= 0
    d_obs = res.score_stat[known]
    both = np.isfinite(d_obs) & np.isfinite(h_obs)
    gap_obs = float(np.max(np.abs(d_obs / h_obs - 1)[both]))
    o_obs = host_omnibus(features(plan, True), omni_sets, plan.y.astype(np.float64), covar)
    o_both = np.isfinite(omni.score_stat) & np.isfinite(o_obs) & (omni.flags == 0)
    gap_omni = float(np.max(np.abs(omni.score_stat / o_obs - 1)[o_both]))
    q_dev, q_host = float(np.quantile(res.min_p, 0.05)), float(np.quantile(h_minp, 0.05))
    spread = 4.0 * math.sqrt(2 * 0.05 * 0.95 / a.perms) / 0.05
    close = bool(both.sum() >= 0.9 * len(h_obs) and np.array_equal(np.isfinite(d_obs), np.isfinite(h_obs)) and gap_obs <= 1e-9
                 and o_both.sum() >= 0.9 * len(o_obs) and gap_omni <= 1e-9 and abs(q_dev / q_host - 1) <= spread)
    best, host = single["e2e_s"], min(host_s)
    top = int(np.nanargmax(res.score_stat))
    print(json.dumps({
        "tool": "assocscore_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "tests": len(res.name), "covariates": a.covariates, "model": "dominant", "perms": a.perms,
        "assoc_score_s": best, "single": single, "omnibus": omnibus,
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / single["device_part_s"], 1),
        "compared": int(both.sum()), "observed_gap": gap_obs, "omnibus_compared": int(o_both.sum()), "omnibus_observed_gap": gap_omni,
        "min_p_q05_device": q_dev, "min_p_q05_host": q_host, "q05_spread_allowed": round(spread, 3),
        "top": res.name[top], "top_score_p": float(res.score_p[top]), "top_perm_p_adj": float(res.perm_p_adj[top]),
        "bonferroni_top": float(min(1.0, res.score_p[top] * np.isfinite(res.score_p).sum())), "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
