#!/usr/bin/env python3
"""hlaOutOfBagEnsemble against the per-sample hand loop on the existing API: for every training sample the sub-model of
its out-of-bag classifiers -> hlaModelFromObj -> hlaPredict(type="response") -> hlaClose.  Workload: the synthetic HLA-B
model (100 classifiers) with 1,000 training samples and a seeded bootstrap (bincount of n draws per classifier).  The loop
is timed on the first `loop_samples` samples and scaled to the cohort (the output says so); on those samples the two
results are asserted bit-equal.  Prints one JSON line.

Usage: python tools/oobens_bench.py [n_samp] [loop_samples] [repeats] [--loop-only]
--loop-only: time the hand loop alone (what a build of the library without hibag_hip_predict_masked, selected with
HIBAG_HIP_LIBRARY, can run: the loop uses nothing new)."""
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hibag_amd as hb                      # noqa: E402
from hibag_amd import synth                  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
loop_only = "--loop-only" in sys.argv
n_samp = int(args[0]) if len(args) > 0 else 1000
n_loop = min(n_samp, int(args[1]) if len(args) > 1 else 100)
reps = int(args[2]) if len(args) > 2 else 5
hb.hlaSetKernelTarget("hip")
obj, founders, af = synth.make_model("hla-b")
G, truth = synth.make_samples(founders, af, n_samp, seed=10)
snp = synth.as_snp_geno(obj, G)
obj.sample_id = list(snp.sample_id)
obj.n_samp = n_samp
rng = np.random.default_rng(11)
for c in obj.classifiers:
    c.samp_num = np.bincount(rng.integers(0, n_samp, n_samp), minlength=n_samp).astype(np.int32)
hla = hb.hlaAllele(snp.sample_id, [obj.hla_allele[a] for a in truth[:, 0]], [obj.hla_allele[a] for a in truth[:, 1]], locus="B")
use = np.stack([c.samp_num for c in obj.classifiers]) == 0
geno = np.asarray(snp.genotype)


def hand_loop():
    h1, h2, prob, matching = [], [], [], []
    for s in range(n_loop):
        sub = dataclasses.replace(obj, classifiers=[c for c, u in zip(obj.classifiers, use[:, s]) if u])
        m = hb.hlaModelFromObj(sub)
        v = hb.hlaPredict(m, geno[:, s], type="response", verbose=False)
        hb.hlaClose(m)
        h1.append(v.h1[0]); h2.append(v.h2[0]); prob.append(v.prob[0]); matching.append(v.matching[0])
    return np.array(h1), np.array(h2), np.array(prob), np.array(matching)


def best(f):
    f()                                                   # (warm-up)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return min(ts), out


t_loop, loop = best(hand_loop)
line = {"n_classifier": len(obj.classifiers), "n_samp": n_samp, "oob_classifiers_min": int(use.sum(0).min()),
        "oob_classifiers_max": int(use.sum(0).max()), "loop_samples": n_loop, "hand_loop_measured_s": t_loop,
        "hand_loop_scaled_s": t_loop * n_samp / n_loop,
        "note": f"hand loop timed on the first {n_loop} samples, scaled by {n_samp}/{n_loop}"}
if not loop_only:
    model = hb.hlaModelFromObj(obj)
    t_ens, got = best(lambda: hb.hlaOutOfBagEnsemble(model, hla, snp, verbose=False))
    G_model = np.ascontiguousarray(geno.T, np.int32)
    t_call, _ = best(lambda: model.predict_masked(G_model, use, want_dosage=False))
    p = got["pred"]
    for name, a, b in (("h1", p.h1, loop[0]), ("h2", p.h2, loop[1]), ("prob", p.prob, loop[2]), ("matching", p.matching, loop[3])):
        a, b = np.ascontiguousarray(a[:n_loop]), np.ascontiguousarray(b)
        same = np.array_equal(a, b) if a.dtype.kind == "i" else bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
        assert same, f"hlaOutOfBagEnsemble and the hand loop differ in '{name}'"
    model.close()
    line.update({"hlaOutOfBagEnsemble_s": t_ens, "predict_masked_call_s": t_call, "speedup": line["hand_loop_scaled_s"] / t_ens,
                 "bit_equal_on_loop_samples": True, "acc_haplo": got["overall"]["acc.haplo"],
                 "live_pass1_pairs": float(np.mean([use[:, g:g + 64].any(axis=1).mean() for g in range(0, n_samp, 64)]))})
print(json.dumps(line))
