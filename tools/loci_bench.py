#!/usr/bin/env python3
"""Multi-locus typing of one cohort: the per-locus hlaPredict loop against hlaPredictLoci, on a fresh cohort (host object
in, temporary resident cohort inside the call) and on a resident one (HlaDeviceCohort built once, outside the timed
region).  Four synthetic loci of different shapes (synth.make_model: the small HLA-A shape, HLA-B, a model with wide
classifiers, HLA-DRB1) on disjoint SNP sets over ONE cohort of 1,000 SNPs -- five times what the largest model uses -- at
10,000 and at 100,000 samples.  Every timed call is compared bit for bit with the loop's result.

Each measurement runs in a child process of its own under a time limit (warm-up, then the median of the repeats); the three
routes are interleaved and the whole round is repeated (default three times); the figure reported is the median of the
rounds' medians.  `--loop-library PATH` times the loop on another build of the library (the parent commit's: the loop must
not be timed on the tree under test; this tree's Python drives it, the package binds an older library without the cohort
entries).  A route whose results differ from the loop's fails the run.  The byte counts are arithmetic on the shapes (4 bytes
per genotype of every row a route sends; the resident cohort reports its own upload), not counters.  Prints one JSON line.
Usage: python tools/loci_bench.py [--samples 10000,100000] [--reps 7] [--rounds 3] [--loop-library PATH] [--timeout 300]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_COHORT_SNP = 1000
LOCI = [("A", "hla-a-small", dict(seed=101)),
        ("B", "hla-b", dict(seed=102)),
        ("W", "hla-b", dict(seed=103, n_snp=160, n_classifier=14, snp_counts=[12, 113, 18, 40, 24, 30, 31, 32, 56, 84, 100, 120, 128, 20])),
        ("DRB1", "hla-drb1", dict(seed=104))]


def make_case(n_samp):
    """{locus: model}, the cohort as an HlaSNPGeno [1,000 SNPs, n_samp] in numpy's row-major order (SNPs shuffled)."""
    import hibag_amd as hb
    from hibag_amd import synth
    rng = np.random.default_rng(7)
    models, rows, ids, pos = {}, [], [], []
    for li, (locus, shape, kw) in enumerate(LOCI):
        model, founders, af = synth.make_model(shape, **kw)
        model.hla_locus = locus
        model.snp_position = model.snp_position + 1_000_000 * li
        model.snp_id = [f"{locus}_{s}" for s in model.snp_id]
        G, _ = synth.make_samples(founders, af, n_samp, seed=200 + li)
        rows.append(G.T); ids += model.snp_id; pos += list(model.snp_position)
        models[locus] = model
    extra = N_COHORT_SNP - len(ids)
    rows.append(rng.integers(0, 3, (extra, n_samp), dtype=np.int32)); ids += [f"x{e}" for e in range(extra)]
    pos += [1000.0 + e for e in range(extra)]
    order = rng.permutation(N_COHORT_SNP)
    mat = np.concatenate(rows, axis=0)[order]
    snp = hb.HlaSNPGeno(genotype=np.ascontiguousarray(mat, np.int32), sample_id=[f"s{i}" for i in range(n_samp)],
                        snp_id=[ids[i] for i in order], snp_position=np.array(pos, np.float64)[order],
                        snp_allele=["A/G"] * N_COHORT_SNP, assembly="hg19")
    return models, snp


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in ("h1", "h2", "prob", "matching", "dosage"))


def child(route, n_samp, reps):
    import hibag_amd as hb
    hb.hlaSetKernelTarget("hip")
    models, snp = make_case(n_samp)
    dev = {k: hb.hlaModelFromObj(m) for k, m in models.items()}

    def loop():
        return {k: hb.hlaPredict(m, snp, verbose=False) for k, m in dev.items()}
    want = loop()
    out = {"route": route, "n_samp": n_samp, "reps": reps,
           "bytes_loop": int(sum(4 * n_samp * m.n_snp for m in models.values()))}
    cohort = None
    if route == "loop":
        run = loop
    elif route == "fresh":
        def run():
            return hb.hlaPredictLoci(dev, snp, verbose=False)
        out["bytes_fresh"] = int(4 * n_samp * sum(m.n_snp for m in models.values()))
    else:
        t = time.perf_counter()
        cohort = hb.HlaDeviceCohort(snp)
        out["cohort_build_s"] = time.perf_counter() - t
        out["bytes_cohort_build"] = int(cohort.uploaded_bytes)
        out["cohort_device_bytes"] = int(cohort.nbytes)
        out["bytes_resident_call"] = int(sum(8 * m.n_snp for m in models.values()))

        def run():
            return hb.hlaPredictLoci(dev, cohort, verbose=False)
    got = run()                                         # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        got = run()
        ts.append(time.perf_counter() - t)
    out["median_s"] = float(np.median(ts))
    out["min_s"] = float(np.min(ts))
    out["bit_equal"] = bool(all(same(got[k], want[k]) for k in dev))
    out["faults"] = int(sum(m.handover_faults() for m in dev.values()))
    assert out["bit_equal"], f"{route}: the results differ from the per-locus loop's"
    if cohort is not None:
        cohort.close()
    for m in dev.values():
        m.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="10000,100000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-library", default=None)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.reps)
        return
    res = {"cohort_snps": N_COHORT_SNP, "loci": [k for k, _, _ in LOCI], "reps": a.reps, "rounds": a.rounds,
           "loop_library": a.loop_library or "this build", "sizes": {}}
    for n in [int(x) for x in a.samples.split(",")]:
        runs = {"loop": [], "fresh": [], "resident": []}
        for _ in range(a.rounds):
            for route in ("loop", "fresh", "resident"):
                env = dict(os.environ)
                if route == "loop" and a.loop_library:
                    env["HIBAG_HIP_LIBRARY"] = os.path.abspath(a.loop_library)
                # a fresh child per device step, under its own time limit; a failing step ends the run
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", route, str(n)],
                                       env=env, capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"error": f"{route} at {n} samples ran into the time limit of {a.timeout} s"}))
                    sys.exit(1)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(json.dumps({"error": f"{route} at {n} samples exited with {p.returncode}", "stderr": p.stderr[-2000:]}))
                    sys.exit(1)
                runs[route].append(json.loads(line[-1][7:]))
        med = {r: float(np.median([x["median_s"] for x in v])) for r, v in runs.items()}
        last = runs["resident"][-1]
        res["sizes"][str(n)] = {
            "loop_s": med["loop"], "loci_fresh_s": med["fresh"], "loci_resident_s": med["resident"],
            "rounds": {r: [x["median_s"] for x in v] for r, v in runs.items()},
            "fresh_over_loop": med["fresh"] / med["loop"], "loop_over_resident": med["loop"] / med["resident"],
            "cohort_build_s": float(np.median([x["cohort_build_s"] for x in runs["resident"]])),
            "bytes_loop": runs["loop"][-1]["bytes_loop"], "bytes_fresh": runs["fresh"][-1]["bytes_fresh"],
            "bytes_cohort_build": last["bytes_cohort_build"], "bytes_resident_call": last["bytes_resident_call"],
            "cohort_device_bytes": last["cohort_device_bytes"],
            "bit_equal": bool(all(x["bit_equal"] for v in runs.values() for x in v)),
            "faults": int(sum(x["faults"] for v in runs.values() for x in v)),
        }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
