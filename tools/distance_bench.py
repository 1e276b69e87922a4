#!/usr/bin/env python3
"""hlaDistance on the device against the CPU restatement of tests/distance_reference.py (numpy, sequential cumsum per
cell) on the HLA-B and DRB1 shapes and a wide one (200 alleles, 2,000 haplotypes per classifier).  Per shape: end to end
seconds of hlaDistance on an HlaAttrBagClass (median of the repeats), the event time of its kernels, the CPU reference's
seconds, the longest chain of dependent adds (pairs of the largest cell), and whether every output bit matched.
Prints one JSON line.  Usage: python tools/distance_bench.py [repeats]"""
import json
import os
import sys
import time
import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hibag_amd as hb                      # noqa: E402
from hibag_amd import _lib, synth            # noqa: E402
import distance_reference as R              # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
SHAPES = {
    "hla-b": ("hla-b", {}),
    "hla-drb1": ("hla-drb1", {}),
    "wide": ("hla-drb1", dict(n_hla=200, n_haplo=2000, n_classifier=20)),
}


def longest_cell(model):
    best = 0
    for c in model.classifiers:
        cnt = np.bincount(c.hla, minlength=model.n_hla).astype(np.int64)
        cnt = cnt[cnt > 0]
        best = max(best, int(cnt.max() * (cnt.max() + 1) // 2), int(np.sort(cnt)[-2:].prod()) if len(cnt) > 1 else 0)
    return best


def same_bits(a, b):
    if not np.array_equal(a, b, equal_nan=True):
        return False
    k = ~np.isnan(a)
    return np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))


hb.hlaSetKernelTarget("hip")
L = _lib.lib()
res = {"reps": reps}
for name, (shape, over) in SHAPES.items():
    model, _, _ = synth.make_model(shape, **over)
    dev = hb.hlaModelFromObj(model)
    got, each = hb.hlaDistance(dev, classifiers=True)          # warm-up (and the per-classifier matrices)
    e2e, kern = [], []
    for _ in range(reps):
        t = time.perf_counter()
        out = hb.hlaDistance(dev)
        e2e.append(time.perf_counter() - t)
        ms = C.c_double()
        _lib.check(L.hibag_hip_model_distance_ms(dev.handle, C.byref(ms)))
        kern.append(ms.value / 1e3)
        if not same_bits(out, got):
            raise SystemExit(f"{name}: repeated calls differ")
    t = time.perf_counter()
    want, want_each = R.distance(model)
    t_cpu = time.perf_counter() - t
    dev.close()
    res[name] = {
        "n_hla": model.n_hla, "n_classifier": len(model.classifiers), "n_haplo": len(model.classifiers[0].hla),
        "pairs": int(sum(len(c.hla) * (len(c.hla) + 1) // 2 for c in model.classifiers)),
        "longest_chain_pairs": longest_cell(model),
        "gpu_e2e_s": float(np.median(e2e)), "kernel_s": float(np.median(kern)), "cpu_reference_s": t_cpu,
        "bit_equal": bool(same_bits(got, want) and same_bits(each, want_each)),
    }
res["bit_equal"] = all(res[k]["bit_equal"] for k in SHAPES)
print(json.dumps(res))
