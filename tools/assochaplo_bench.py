#!/usr/bin/env python3
"""hlaAssocHaplo at scale: one JSON line.

    python tools/assochaplo_bench.py [--samples 10000] [--loci 4] [--k 3] [--covariates 6] [--perms 10000] [--min-freq 0.01]
                                     [--reps 3] [--gram-rows 346] [--no-host-em]

The workload of tools/haplo_bench.py (10,000 synthetic samples x 4 loci x k = 3 drawn from a pool of 40 haplotypes with linkage
disequilibrium) through ``hlaHaplotypes(..., dosage_min_freq=min_freq)``, a case / control label with a planted effect of the
most frequent haplotype's expected dosage and 6 standard-normal covariates, then ``hlaAssocHaplo`` with 10,000 sign
replicates.  Timed, best of --reps: hlaHaplotypes with and without the dosages, the dosage call alone, hlaAssocHaplo end to
end, its device part, and the event times of the resampling call (residual panels, ``k_rscore_gram``, statistics).
``--gram-rows`` random real rows on the same handle give ``k_rscore_gram``'s event time at the panel of DESIGN.md section
28's timing (346 rows x 10,000 samples x 10,000 replicates), where ``k_quant_gram`` takes 2.48 ms.

The host baseline does the association the way a user would in numpy on at most 16 threads (tools/assocscore_bench.py's:
IRLS, QR of the weighted covariates, an explicit sign matrix, one float64 matrix product per 1,000 replicates) on the same
dosages, timed in the same run; the two sides are compared on the observed statistics (1e-9 relative) and on the 5 % point
of the replicates' smallest p-value within its sampling error.  Unless --no-host-em, the dosages themselves are compared
with those of tools/haplo_bench.py's numpy EM (np.bincount over (haplotype, sample)), to 1e-9."""

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
from hibag_amd import assoc, assocscore, haplo  # noqa: E402
from hibag_amd.topk import HlaTopCalls  # noqa: E402
from assocscore_bench import host_baseline  # noqa: E402
from haplo_bench import cohort, host_em, host_states  # noqa: E402


def best(f, reps):
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = f()
        out.append(time.perf_counter() - t0)
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--loci", type=int, default=4)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--pool", type=int, default=40)
    ap.add_argument("--alleles", type=int, default=30)
    ap.add_argument("--covariates", type=int, default=6)
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--min-freq", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gram-rows", type=int, default=346)
    ap.add_argument("--no-host-em", action="store_true")
    a = ap.parse_args()
    n, L, k = a.samples, a.loci, a.k
    _, h1, h2, prob = cohort(n, L, k, a.pool, a.alleles, 1)
    ids = [f"s{i}" for i in range(n)]
    calls = {f"L{l}": HlaTopCalls(f"L{l}", ids, k, h1[l], h2[l], prob[l], np.ones(n), levels=[f"L{l}*{i:02d}" for i in range(a.alleles)])
             for l in range(L)}
    kw = dict(min_prob=0.0, maxit=200, tol=1e-8, verbose=False)
    seed = 20241021

    hb.hlaHaplotypes(calls, dosage_min_freq=a.min_freq, **kw)                  # warm-up: code objects, allocations
    _, plain_s = best(lambda: hb.hlaHaplotypes(calls, **kw), a.reps)
    res, with_s = best(lambda: hb.hlaHaplotypes(calls, dosage_min_freq=a.min_freq, **kw), a.reps)
    with haplo._DeviceHaplo(h1, h2, prob, 4096) as dev:
        fit = dev.fit(200, 1e-8)
        order = np.lexsort((fit["keys"], -fit["freq"]))
        _, dosage_s = best(lambda: dev.dosage(order[res.dosage_index]), a.reps)
    m = len(res.dosage_index)

    rng = np.random.default_rng(7)
    covar = rng.standard_normal((n, a.covariates))
    eta = -0.4 + 0.5 * res.dosage[0] + 0.2 * covar[:, 0]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)

    hb.hlaAssocHaplo(res, y, covar, min_freq=a.min_freq, n_perm=64, seed=seed)
    out, e2e = best(lambda: hb.hlaAssocHaplo(res, y, covar, min_freq=a.min_freq, n_perm=a.perms, seed=seed), a.reps)
    omni, omni_s = None, [float("nan")]
    if m <= assocscore.MAX_ROWS:
        omni, omni_s = best(lambda: hb.hlaAssocHaplo(res, y, covar, min_freq=a.min_freq, omnibus=True, n_perm=a.perms, seed=seed), a.reps)

    # the device part alone, and the kernels' event times
    hla = res.as_alleles(a.min_freq)
    plan = assoc._Plan(hla, y, float("nan"), None)
    D = np.ascontiguousarray(res.dosage[:, plan.sel])
    cov_t = np.ascontiguousarray(covar[plan.sel].T)
    sets = [[j] for j in range(m)]
    dev_s, res_s, ms = [], [], []
    wide = rng.uniform(0.0, 2.0, (a.gram_rows, plan.n_samp)) * (rng.random((a.gram_rows, plan.n_samp)) < 0.5)
    wide_ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assocscore._DeviceScore(plan.a1, plan.a2, plan.y, len(plan.alleles), None, 0) as sdev:
            sdev.score(cov_t, None, 25, 1e-8)
            sdev.score_real_sets(D, sets)
            t1 = time.perf_counter()
            sdev.score_resample(seed, 1, a.perms)
            res_s.append(time.perf_counter() - t1)
            ms.append(sdev.score_ms())
            dev_s.append(time.perf_counter() - t0)
            sdev.score_real_sets(wide, [[j] for j in range(a.gram_rows)])
            sdev.score_resample(seed, 1, a.perms)
            wide_ms.append(sdev.score_ms())
    kbest = int(np.argmin([sum(x) for x in ms]))

    # the host's analysis of the same definition on the same dosages
    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_obs, h_minp = host_baseline(D, plan.y.astype(np.float64), covar[plan.sel], a.perms, seed)
        host_s.append(time.perf_counter() - t0)
    both = np.isfinite(out.score_stat) & np.isfinite(h_obs)
    gap_obs = float(np.max(np.abs(out.score_stat / h_obs - 1)[both]))
    q_dev, q_host = float(np.quantile(out.min_p, 0.05)), float(np.quantile(h_minp, 0.05))
    spread = 4.0 * math.sqrt(2 * 0.05 * 0.95 / a.perms) / 0.05
    close = bool(both.all() and gap_obs <= 1e-9 and abs(q_dev / q_host - 1) <= spread)

    dosage_gap = None
    host_dosage_s = None
    if not a.no_host_em:
        wc, ka, kb, samp = host_states(h1, h2, prob)
        keys, f, it, delta, q, iA, iB = host_em(wc, ka, kb, samp, n, 200, 1e-8)
        t0 = time.perf_counter()
        want = np.zeros((m, n))
        for r, key in enumerate(res.keys[res.dosage_index].astype(np.int64)):
            h = int(np.searchsorted(keys, key))
            for idx in (iA, iB):
                at = idx == h
                want[r] += np.bincount(samp[at], q[at], n)
        host_dosage_s = time.perf_counter() - t0
        dosage_gap = float(np.abs(want - res.dosage).max())
        close = close and dosage_gap <= 1e-9

    top = int(np.nanargmax(out.score_stat))
    print(json.dumps({
        "tool": "assochaplo_bench", "samples": n, "loci": L, "k": k, "states": int(res.n_states.sum()), "haplotypes": len(res.freq),
        "tested": m, "covariates": a.covariates, "perms": a.perms, "min_freq": a.min_freq,
        "haplotypes_s": round(min(plain_s), 5), "haplotypes_with_dosage_s": round(min(with_s), 5), "dosage_call_s": round(min(dosage_s), 5),
        "assoc_haplo_s": round(min(e2e), 5), "assoc_haplo_s_all": [round(x, 5) for x in e2e], "omnibus_s": None if omni is None else round(min(omni_s), 5),
        "omnibus_df": None if omni is None else int(omni.df[0]), "device_part_s": round(min(dev_s), 5), "resample_call_s": round(min(res_s), 5),
        "project_ms": round(ms[kbest][0], 3), "rscore_gram_ms": round(ms[kbest][1], 3), "stat_ms": round(ms[kbest][2], 3),
        "gram_rows": a.gram_rows, "rscore_gram_ms_at_gram_rows": round(min(x[1] for x in wide_ms), 3),
        "host_baseline_s": round(min(host_s), 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(min(host_s) / min(e2e), 1), "host_threads": int(os.environ["OMP_NUM_THREADS"]),
        "observed_gap": gap_obs, "min_p_q05_device": q_dev, "min_p_q05_host": q_host, "q05_spread_allowed": round(spread, 3),
        "dosage_gap_vs_host_em": dosage_gap, "host_dosage_s": None if host_dosage_s is None else round(host_dosage_s, 4),
        "top": out.name[top], "top_is_planted": bool(top == 0), "top_score_p": float(out.score_p[top]),
        "top_perm_p_adj": float(out.perm_p_adj[top]), "close": close}))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
