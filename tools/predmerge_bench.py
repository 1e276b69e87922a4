#!/usr/bin/env python3
"""hlaPredictMerge against the route it replaces -- k x hlaPredict(type="response+prob") + hlaPredMerge on the host -- for
k = 2 and k = 4 HLA-B-shaped models x 10,000 samples, both in this process on the same device.  Per k: the median and the
spread (min, max) of the repeats of each route after a warm-up, their ratio, whether the two results are identical bit for
bit, the sum of the k plain hlaPredict(type="response+dosage") times (what the merge adds on top of the predictions), and
the device time of the merge alone on materialised sample-major posteriors (hibag_hip_merge_device, HIP events) -- the
layout the fused call avoids.  Prints one JSON line.  Usage: python tools/predmerge_bench.py [repeats] [samples]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()                            # (before the library's own HIP context: torch's lazy initialisation fails after it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hibag_amd as hb                      # noqa: E402
from hibag_amd import _lib, synth            # noqa: E402
from hibag_amd.merge import merge_plan       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
n_samp = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000


def timed(fn, n):
    fn()                                     # warm-up
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = fn()
        t.append(time.perf_counter() - t0)
    return r, {"median_s": float(np.median(t)), "min_s": float(min(t)), "max_s": float(max(t))}


def bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def merge_device_ms(devs, objs, geno):
    """Event time of hibag_hip_merge_device on the k posterior matrices hibag_hip_predict_device wrote."""
    dev = torch.device("cuda", devs[0].device())
    k, n = len(devs), geno.shape[0]
    d_geno = torch.from_numpy(geno).to(dev)
    pp = [torch.empty((n, o.n_cell), dtype=torch.float64, device=dev) for o in objs]
    mt = [torch.empty(n, dtype=torch.float64, device=dev) for _ in objs]
    st = torch.cuda.current_stream(dev)
    for m, p, t in zip(devs, pp, mt):
        m.predict_device(d_geno.data_ptr(), n, 1, d_matching=t.data_ptr(), d_postprob=p.data_ptr(), stream=st.cuda_stream)
    plan = merge_plan([o.hla_allele for o in objs])
    maps = [np.ascontiguousarray(r, np.int32) for r in plan.row_of_cell]
    L = _lib.lib()
    h = C.c_void_p(L.hibag_hip_merge_plan_new(k, np.array([len(r) for r in maps], np.int32).ctypes.data_as(C.c_void_p),
                                              (C.c_void_p * k)(*[r.ctypes.data for r in maps]), len(plan.hla_allele), devs[0].device()))
    h1, h2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    pb, mo = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    ds = torch.empty((len(plan.hla_allele), n), dtype=torch.float64, device=dev)
    w = np.full(k, 1.0 / k)
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        _lib.check(L.hibag_hip_merge_device(h, (C.c_void_p * k)(*[p.data_ptr() for p in pp]), (C.c_void_p * k)(*[t.data_ptr() for t in mt]),
                                            w.ctypes.data_as(C.c_void_p), 1, n, C.c_void_p(h1.data_ptr()), C.c_void_p(h2.data_ptr()),
                                            C.c_void_p(pb.data_ptr()), C.c_void_p(mo.data_ptr()), C.c_void_p(ds.data_ptr()), None, n,
                                            C.c_void_p(st.cuda_stream)))
        b.record(st)
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    L.hibag_hip_merge_plan_free(h)
    return float(np.median(ms[1:]))


hb.hlaSetKernelTarget("hip")
res = {"reps": reps, "n_samp": n_samp, "shape": "hla-b"}
ok = True
for k in (2, 4):
    objs, devs, first = [], [], None
    for i in range(k):
        obj, founders, afreq = synth.make_model("hla-b", seed=synth.DEFAULT_SEED + 31 * i)
        obj.hla_allele = [f"{60 + a}:01" if (a + i) % 5 == 0 and i else x for a, x in enumerate(obj.hla_allele)]   # overlapping sets
        obj.hla_locus = "B"
        first = first or (founders, afreq)
        objs.append(obj)
        devs.append(hb.hlaModelFromObj(obj))
    geno, _ = synth.make_samples(first[0], first[1], n_samp)
    snp = synth.as_snp_geno(objs[0], geno)

    def composed():
        return hb.hlaPredMerge(*[hb.hlaPredict(m, snp, type="response+prob", verbose=False) for m in devs], verbose=False)

    def fused():
        return hb.hlaPredictMerge(devs, snp, verbose=False)

    def plain():
        return [hb.hlaPredict(m, snp, type="response+dosage", verbose=False) for m in devs]

    got, t_new = timed(fused, reps)
    want, t_old = timed(composed, max(2, reps // 2))
    _, t_plain = timed(plain, reps)
    same = bool(np.array_equal(got.h1, want.h1) and np.array_equal(got.h2, want.h2) and bits(got.prob, want.prob)
                and bits(got.matching, want.matching) and bits(got.dosage, want.dosage))
    ok = ok and same
    res[f"k{k}"] = {"merged_alleles": int(got.dosage.shape[0]), "hlaPredictMerge": t_new, "composed": t_old,
                    "speedup": t_old["median_s"] / t_new["median_s"], "identical": same,
                    "k_plain_hlaPredict": t_plain, "over_plain": t_new["median_s"] / t_plain["median_s"],
                    "merge_device_on_posteriors_ms": merge_device_ms(devs, objs, geno)}
    for m in devs:
        m.close()
res["identical"] = ok
print(json.dumps(res))
