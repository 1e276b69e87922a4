#!/usr/bin/env python3
"""hlaOutOfBag against the literal R loop (R/HIBAG.R:1320-1334) on the existing API: per classifier a one-classifier
hlaModelFromObj + hlaPredict of its out-of-bag samples + hlaCompareAllele(full=True).  Model: trained here on the
tools/train_bench.py data (1,000 samples x 300 SNPs), 100 classifiers.  Checks that both give the same result and
prints one JSON line.  Usage: python tools/oob_bench.py [n_classifier] [n_samp] [n_snp] [repeats]"""
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

n_cls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n_samp = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
n_snp = int(sys.argv[3]) if len(sys.argv) > 3 else 300
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
hb.hlaSetKernelTarget("hip")
base, founders, af = synth.make_model("hla-b", seed=9, n_snp=n_snp, n_classifier=1, wide_classifier=False)
G, truth = synth.make_samples(founders, af, n_samp, seed=10)
snp = synth.as_snp_geno(base, G)
hla = hb.hlaAllele(snp.sample_id, [base.hla_allele[a] for a in truth[:, 0]], [base.hla_allele[a] for a in truth[:, 1]], locus="B")
hb.set_seed(100)
t = time.perf_counter()
model = hb.hlaAttrBagging(hla, snp, nclassifier=n_cls, verbose=False)
t_train = time.perf_counter() - t
obj = model.obj


def r_loop():
    res = []
    for cls in obj.classifiers:
        oob = [i for i, v in enumerate(cls.samp_num) if v == 0]
        m1 = hb.hlaModelFromObj(dataclasses.replace(obj, classifiers=[cls]))
        sub = hb.hlaGenoSubset(snp, samp_sel=[snp.sample_id.index(obj.sample_id[i]) for i in oob])
        v = hb.hlaPredict(m1, sub, verbose=False)
        m1.close()
        res.append(hb.hlaCompareAllele(hla, v, allele_limit=obj, full=True))
    return res


def best(f):
    f()                                                   # (warm-up)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return min(ts), out


t_oob, got = best(lambda: hb.hlaOutOfBag(model, hla, snp, verbose=False))
geno = np.ascontiguousarray(G[[snp.sample_id.index(s) for s in obj.sample_id]][:, [snp.snp_id.index(s) for s in obj.snp_id]])
samp_num = np.stack([np.asarray(c.samp_num, np.int32) for c in obj.classifiers])
t_kernel, _ = best(lambda: model.predict_oob(geno, samp_num))
t_loop, loop = best(r_loop)
conf = sum(r["confusion"] for r in loop) / len(loop)
same = bool(np.array_equal(got["confusion"], conf))
print(json.dumps({"n_classifier": n_cls, "n_samp": n_samp, "n_snp": n_snp, "train_s": t_train,
                  "mean_oob_samples": float(np.mean(np.sum(samp_num == 0, axis=1))),
                  "hlaOutOfBag_s": t_oob, "predict_oob_call_s": t_kernel, "r_loop_s": t_loop,
                  "speedup": t_loop / t_oob, "same_confusion": same,
                  "acc_haplo": got["overall"]["acc.haplo"]}))
