#!/usr/bin/env python3
"""hlaAssocSurv at scale: one JSON line.

    python tools/assocsurv_bench.py [--samples 10000] [--partitions 100] [--covariates 6] [--reps 3]

The cohort of tools/assoc_bench.py (HLA-B-sized allele list, 100 synthetic amino-acid partitions) with 6 standard-normal
covariates that enter the hazard, exponential event times with about 30 % independent censoring, rounded so that about half
the events share their time with another one; the dominant model, Efron's rule: end-to-end seconds of hlaAssocSurv (plan,
sort, device, host columns) and of its device part alone (handle, all fits), best of --reps, against a host baseline that
does the same analysis the way a user would in numpy -- per test a Newton iteration on the partial likelihood, vectorised
over the samples with cumulative sums along the time order (the matrix products through BLAS on at most 16 threads,
numpy.linalg for the solve and the inverse, the same start and stopping rule) -- timed in the same run.  The two sides are
compared on est and se of every test both fitted: 1e-6 in units of max(|est|, se) and 1e-6 relative."""

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
from hibag_amd import assoc, assocsurv  # noqa: E402
from assoc_bench import cohort  # noqa: E402


class Order:
    """What every fit shares: the blocks of equal times (samples in time order, latest first) and the (block, l) pairs."""

    def __init__(self, time, event):
        n = len(time)
        new = np.r_[True, time[1:] != time[:-1]]
        self.starts = np.flatnonzero(new)
        self.last = np.r_[self.starts[1:], n] - 1
        self.blk = np.cumsum(new) - 1
        self.ev = event != 0
        d = np.add.reduceat(self.ev.astype(np.int64), self.starts)
        self.kk = np.flatnonzero(d > 0)
        self.pk = np.repeat(self.kk, d[self.kk])
        self.pstart = np.r_[0, np.cumsum(d[self.kk])[:-1]]
        self.f = (np.arange(len(self.pk)) - np.repeat(self.pstart, d[self.kk])) / d[self.pk]
        self.nb = len(self.starts)


def host_eval(X, O, beta):
    r = np.exp(np.clip(X @ beta, -200.0, 200.0))
    rx = r[:, None] * X
    S0, S1 = np.cumsum(r)[O.last], np.cumsum(rx, axis=0)[O.last]
    D0 = np.add.reduceat(np.where(O.ev, r, 0.0), O.starts)
    D1 = np.add.reduceat(np.where(O.ev[:, None], rx, 0.0), O.starts, axis=0)
    phi = S0[O.pk] - O.f * D0[O.pk]
    v = (S1[O.pk] - O.f[:, None] * D1[O.pk]) / phi[:, None]
    a, b = np.zeros(O.nb), np.zeros(O.nb)
    a[O.kk] = np.add.reduceat(1.0 / phi, O.pstart)
    b[O.kk] = np.add.reduceat(O.f / phi, O.pstart)
    w = r * (np.cumsum(a[::-1])[::-1][O.blk] - np.where(O.ev, b[O.blk], 0.0))
    ll = (X[O.ev] @ beta).sum() - np.log(phi).sum()
    wx = w[:, None] * X
    return ll, X[O.ev].sum(axis=0) - wx.sum(axis=0), X.T @ wx - v.T @ v


def host_fit(X, O, start, maxit=20, epsilon=1e-9):
    """(beta, se) of one Cox regression by Newton's method, or None where it cannot be fitted."""
    beta = start.copy()
    ll, U, info = host_eval(X, O, beta)
    for _ in range(maxit):
        try:
            beta = beta + np.linalg.solve(info, U)
        except np.linalg.LinAlgError:
            return None
        last = info
        ll_new, U, info = host_eval(X, O, beta)
        done = abs(1 - ll / ll_new) <= epsilon
        ll = ll_new
        if done:
            break
    return beta, np.sqrt(np.diag(np.linalg.inv(last)))


def host_baseline(plan, time, covar):
    """est and se [device tests] of the h column, NaN where the column is constant; plan in time order."""
    n = plan.n_samp
    table = np.concatenate([np.arange(len(plan.alleles))[None, :], plan.group_of])
    part = np.concatenate([np.zeros(len(plan.alleles), int)] + [np.full(int(g.max()) + 1, q + 1) for q, g in enumerate(plan.group_of)])
    lev = np.concatenate([np.arange(len(plan.alleles))] + [np.arange(int(g.max()) + 1) for g in plan.group_of])
    F = ((table[part][:, plan.a1] == lev[:, None]) | (table[part][:, plan.a2] == lev[:, None])).astype(np.float64)
    O = Order(time, plan.y)
    covar = covar - covar.mean(axis=0)
    base = host_fit(covar, O, np.zeros(covar.shape[1]))[0]
    X = np.column_stack([np.zeros(n), covar])
    est, se = np.full(len(F), np.nan), np.full(len(F), np.nan)
    for t, h in enumerate(F):
        if h.min() == h.max():
            continue
        X[:, 0] = h
        r = host_fit(X, O, np.r_[0.0, base])
        if r is not None:
            est[t], se[t] = r[0][0], r[1][0]
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
    eta = 0.4 * carrier + covar @ (rng.uniform(-0.4, 0.4, a.covariates))
    t_event = rng.exponential(1.0, a.samples) / np.exp(eta)
    t_cens = rng.exponential(0.7 / 0.3, a.samples)
    event = (t_event <= t_cens).astype(np.int32)
    raw = np.minimum(t_event, t_cens)
    grid = 1.0
    while True:                                                  # the coarsest grid of the ladder on which at most half the events are tied
        tm = np.ceil(raw * grid) / grid
        _, inv, cnt = np.unique(tm[event == 1], return_inverse=True, return_counts=True)
        tied = float((cnt[inv] > 1).mean())
        if tied <= 0.5:
            break
        grid *= 1.1

    hb.hlaAssocSurv(hla, tm, event, covar, groups=groups)               # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = hb.hlaAssocSurv(hla, tm, event, covar, model="dominant", groups=groups)
        e2e.append(time.perf_counter() - t0)
    plan = assoc._Plan(hla, event, float("nan"), groups)
    order = np.argsort(-tm[plan.sel], kind="stable")
    plan.a1, plan.a2, plan.y = (np.ascontiguousarray(v[order]) for v in (plan.a1, plan.a2, plan.y))
    t_sorted, c_sorted = np.ascontiguousarray(tm[plan.sel][order]), covar[plan.sel][order]
    cov_t = np.ascontiguousarray((c_sorted - c_sorted.mean(axis=0)).T)
    dev_s, fit_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with assocsurv._DeviceSurv(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, 0) as dev:
            t1 = time.perf_counter()
            dev.cox(t_sorted, cov_t, 0, 20, 1e-9)
            fit_s.append(time.perf_counter() - t1)
        dev_s.append(time.perf_counter() - t0)

    host_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h_est, h_se = host_baseline(plan, t_sorted, c_sorted)
        host_s.append(time.perf_counter() - t0)

    known = np.array(plan.row) >= 0
    d_est, d_se, d_fl = res.est[known, 0], res.se[known, 0], res.flags[known]
    both = (d_fl == 0) & np.isfinite(h_est)
    gap_est = float(np.max(np.abs(d_est - h_est)[both] / np.maximum(np.abs(h_est), h_se)[both]))
    gap_se = float(np.max(np.abs(d_se / h_se - 1)[both]))
    close = bool(both.sum() >= 0.9 * len(h_est) and gap_est <= 1e-6 and gap_se <= 1e-6)
    best, host = min(e2e), min(host_s)
    print(json.dumps({
        "tool": "assocsurv_bench", "samples": a.samples, "alleles": len(plan.alleles), "partitions": a.partitions,
        "tests": len(res.name), "covariates": a.covariates, "model": "dominant", "ties": "efron",
        "events": int(event.sum()), "censored_fraction": round(1 - float(event.mean()), 3), "tied_event_fraction": round(tied, 3),
        "distinct_times": int(len(np.unique(tm))),
        "assoc_surv_s": round(best, 5), "assoc_surv_s_all": [round(x, 5) for x in e2e],
        "device_part_s": round(min(dev_s), 5), "device_fits_s": round(min(fit_s), 5),
        "host_baseline_s": round(host, 4), "host_baseline_s_all": [round(x, 4) for x in host_s],
        "speedup_vs_host": round(host / best, 1), "device_part_speedup": round(host / min(dev_s), 1),
        "iterations_max": int(res.iterations.max()), "compared": int(both.sum()),
        "est_gap": gap_est, "se_gap": gap_se, "close": close,
    }))
    return 0 if close else 1


if __name__ == "__main__":
    sys.exit(main())
