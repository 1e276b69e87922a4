#!/usr/bin/env python3
"""hlaLDMatrix / hlaGenoLD at scale: one JSON line.

    python tools/ld_bench.py [--samples 10000] [--snps 5000] [--alleles 60] [--reps 3]

hlaLDMatrix on a seeded synthetic cohort (NAs in 3 % of the samples): end-to-end seconds of the call (it returns after
the last panel is on the host, i.e. after a device synchronise), the event time of its Gram kernels, the Gram's share of
the int8 dense matrix peak, and the device-to-host rate of the result; the float64-BLAS reference of tests/ld_reference.py
on at most 16 threads, timed in the same run, with a check that both outputs are equal bit for bit; hlaGenoLD at the same
size with --alleles alleles."""

import argparse
import json
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(int(os.environ.get(v, "16")), 16))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import hibag_amd as hb  # noqa: E402
import ld_reference as R  # noqa: E402
from hibag_amd.ld import _DeviceGeno  # noqa: E402

I8_DENSE_PEAK_OPS = 5.0e15      # MI355X int8 dense matrix peak (2 ops per multiply-add), about 2x the BF16 rate


def cohort(n_snp, n_samp, seed=2024):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.int32)
    na_samp = rng.choice(n_samp, n_samp * 3 // 100, replace=False)
    g[rng.integers(0, n_snp, na_samp.size), na_samp] = hb.NA_INTEGER
    return g, rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=5000)
    ap.add_argument("--alleles", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    g, rng = cohort(a.snps, a.samples)
    geno = hb.HlaSNPGeno(genotype=g, sample_id=[f"s{i}" for i in range(a.samples)], snp_id=[f"rs{j}" for j in range(a.snps)])

    hb.hlaLDMatrix(geno, maf=0.01, draw=False, verbose=False)              # warm-up: code objects, allocations
    e2e = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        got = hb.hlaLDMatrix(geno, maf=0.01, draw=False, verbose=False)
        e2e.append(time.perf_counter() - t0)
    # the Gram's event time and the panel copies, from one more call on a handle of our own
    t0 = time.perf_counter()
    with _DeviceGeno(g) as dg:
        t_upload = time.perf_counter() - t0
        n_valid, s = dg.snp_counts()
        keep = R.maf_keep(g, 0.01)
        t0 = time.perf_counter()
        _, n_c = dg.matrix(keep)
        t_matrix = time.perf_counter() - t0
        gram_ms = dg.gram_ms()
    k = len(keep)
    ops = 2.0 * k * k * (-(-n_c // 128) * 128)

    t0 = time.perf_counter()
    want, _ = R.ld_matrix(g[keep])
    t_ref = time.perf_counter() - t0
    equal = bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))

    names = [f"{i:03d}:01" for i in range(a.alleles)]
    a1 = [names[i] for i in rng.integers(0, a.alleles, a.samples)]
    a2 = [names[i] for i in rng.integers(0, a.alleles, a.samples)]
    hla = hb.HlaAlleleClass(locus="A", sample_id=geno.sample_id, allele1=a1, allele2=a2)
    hb.hlaGenoLD(hla, geno)
    t_geno = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ld = hb.hlaGenoLD(hla, geno)
        t_geno.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want_ld = R.geno_ld(g, a1, a2)[0]
    t_geno_ref = time.perf_counter() - t0
    geno_equal = bool(np.array_equal(ld.view(np.uint64), want_ld.view(np.uint64)))

    best = min(e2e)
    print(json.dumps({
        "tool": "ld_bench", "samples": a.samples, "snps": a.snps, "kept_snps": k, "complete_samples": n_c,
        "ld_matrix_s": round(best, 5), "ld_matrix_s_all": [round(x, 5) for x in e2e],
        "upload_pack_s": round(t_upload, 5), "matrix_call_s": round(t_matrix, 5), "gram_ms": round(gram_ms, 4), "gram_i8_peak_share": round(ops / (gram_ms * 1e-3) / I8_DENSE_PEAK_OPS, 4) if gram_ms else None,
        "result_gb": round(8.0 * k * k / 1e9, 4), "d2h_gb_per_s": round(8.0 * k * k / 1e9 / t_matrix, 2),
        "blas_reference_s": round(t_ref, 4), "speedup_vs_blas": round(t_ref / best, 1), "outputs_equal": equal,
        "geno_ld_alleles": a.alleles, "geno_ld_s": round(min(t_geno), 5), "geno_ld_reference_s": round(t_geno_ref, 4),
        "geno_ld_equal": geno_equal,
    }))
    return 0 if equal and geno_equal else 1


if __name__ == "__main__":
    sys.exit(main())
