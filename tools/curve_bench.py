#!/usr/bin/env python3
"""hlaPredictCurve against the hand loop on the same device, at the headline shape (synthetic HLA-B, 100 classifiers,
10,000 samples, all 100 sizes).  The loop is the reference's way: per size hlaSubModelObj -> hlaModelFromObj ->
hlaPredict(type="response") -> hlaClose.  Both are timed end to end (host calls included; medians of the repeats after a
warm-up of each), the event time of k_prefix_accum comes from the library, and every call, probability and matching
proportion of the two is compared bit for bit.  Prints one JSON line.
Usage: python tools/curve_bench.py [samples [curve repeats [loop repeats]]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hibag_amd as hb                      # noqa: E402
from hibag_amd import synth                  # noqa: E402

n_samp = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
loop_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2


def same_bits(a, b):
    if not np.array_equal(a, b, equal_nan=True):
        return False
    k = ~np.isnan(a)
    return np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))


hb.hlaSetKernelTarget("hip")
model, founders, af = synth.make_model("hla-b")
G, _ = synth.make_samples(founders, af, n_samp)
snp = synth.as_snp_geno(model, G)
K = len(model.classifiers)
dev = hb.hlaModelFromObj(model)


def hand_loop():
    out = []
    for k in range(1, K + 1):
        m = hb.hlaModelFromObj(hb.hlaSubModelObj(model, k))
        out.append(hb.hlaPredict(m, snp, type="response", verbose=False))
        hb.hlaClose(m)
    return out


curve = hb.hlaPredictCurve(dev, snp, verbose=False)              # warm-up: builds the second layout
t_curve, t_accum = [], []
for _ in range(reps):
    t = time.perf_counter()
    curve = hb.hlaPredictCurve(dev, snp, verbose=False)
    t_curve.append(time.perf_counter() - t)
    t_accum.append(dev.prefix_accum_ms() / 1e3)
t = time.perf_counter()
tmp = hb.hlaModelFromObj(model)
hb.hlaPredictCurve(tmp, snp, verbose=False)
hb.hlaClose(tmp)
t_cold = time.perf_counter() - t                                  # a fresh model: layout, second layout, one curve

loop = hand_loop()                                               # warm-up
t_loop = []
for _ in range(loop_reps):
    t = time.perf_counter()
    loop = hand_loop()
    t_loop.append(time.perf_counter() - t)

equal = all(np.array_equal(c.h1, r.h1) and np.array_equal(c.h2, r.h2) and same_bits(c.prob, r.prob)
            and same_bits(c.matching, r.matching) for c, r in zip(curve.pred, loop))
probe = hb.hlaModelFromObj(model)
stored_default = probe.stored_cells()
hb.hlaClose(probe)
hb.hlaClose(dev)
res = {
    "shape": "hla-b", "n_classifier": K, "n_samp": n_samp, "n_sizes": K, "reps": reps, "loop_reps": loop_reps,
    "curve_e2e_s": float(np.median(t_curve)), "curve_cold_s": t_cold, "hand_loop_e2e_s": float(np.median(t_loop)),
    "speedup": float(np.median(t_loop) / np.median(t_curve)), "speedup_cold": float(np.median(t_loop) / t_cold),
    "k_prefix_accum_s": float(np.median(t_accum)), "stored_cells_default_layout": int(stored_default),
    "changed_at": {str(int(s)): int(c) for s, c in zip(curve.sizes[[0, 9, 24, 49, 74, K - 1]], curve.changed[[0, 9, 24, 49, 74, K - 1]])},
    "bit_equal": bool(equal),
}
print(json.dumps(res))
