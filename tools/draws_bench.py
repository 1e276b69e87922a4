#!/usr/bin/env python3
"""hlaPredictDraws against what it replaces, on one device, host arrays in and out: the benchmark's HLA-B shape
(100 classifiers, 10,000 samples).  Each figure is the median of repeated calls after warm-up calls:
  draws     hlaPredictDraws(n=10, seed=...)
  loop      hlaPredict(type="response+prob") followed by a vectorised host sampling of the posterior matrix by the same
            contract (tests/draws_reference.py: the Philox uniforms, np.cumsum, one comparison, argmax)
  response  hlaPredict(type="response"): the floor -- what the extra finish is paid on top of
plus the event time of the finish kernels of one call of each from the model's timing API, and an assertion that the two
routes give identical draws.  Prints one JSON line.

--baseline-only: time `loop` and `response` only (a tree that has no hlaPredictDraws, e.g. the parent commit's);
--package DIR: import hibag_amd from DIR instead of this tree (the host sampling always comes from this tree's tests/).
Usage: python tools/draws_bench.py [--baseline-only] [--package DIR] [samples [repeats]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
baseline_only = "--baseline-only" in args
if baseline_only:
    args.remove("--baseline-only")
package = ROOT
if "--package" in args:
    i = args.index("--package")
    package = os.path.abspath(args[i + 1])
    del args[i:i + 2]
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, package)

import hibag_amd as hb                              # noqa: E402
from hibag_amd import synth                          # noqa: E402
from draws_reference import draws_from_postprob      # noqa: E402

n_samp = int(args[0]) if len(args) > 0 else 10_000
reps = int(args[1]) if len(args) > 1 else 9
N = 10
SEED = 20240229
WARM = 2


def timed(f):
    for _ in range(WARM):
        out = f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), out


def finish_ms(dev, f):
    """Event time of the finish kernels of one call of f."""
    dev.set_timing(["finish"])
    dev.reset_timing()
    f()
    ms, n = dev.get_timing()["finish"]
    dev.set_timing(False)
    return ms, n


hb.hlaSetKernelTarget("hip")
shape = "hla-b"
model, founders, af = synth.make_model(shape)
G, _ = synth.make_samples(founders, af, n_samp)
snp = np.asfortranarray(G.T)                  # [n.snp, n.samp] in R's memory order: the C side's sample-major matrix, no copy
dev = hb.hlaModelFromObj(model)
n_hla = model.n_hla


def loop():
    r = hb.hlaPredict(dev, snp, type="response+prob", verbose=False)
    return r, draws_from_postprob(r.postprob.T, N, SEED, 0, n_hla)


def response():
    return hb.hlaPredict(dev, snp, type="response", verbose=False)


t_loop, t_loop_min, (full, want) = timed(loop)
t0 = time.perf_counter()
draws_from_postprob(full.postprob.T, N, SEED, 0, n_hla)
t_sample = time.perf_counter() - t0
t_resp, t_resp_min, resp = timed(response)
res = {"shape": shape, "n_samp": n_samp, "n": N, "seed": SEED, "reps": reps, "warmup": WARM, "baseline_only": baseline_only,
       "package": "this tree" if package == ROOT else "another tree",
       "n_classifier": len(model.classifiers), "n_cell": model.n_cell, "postprob_bytes_per_sample": 8 * model.n_cell,
       "loop_s": t_loop, "loop_min_s": t_loop_min, "loop_host_sampling_s": t_sample,
       "response_s": t_resp, "response_min_s": t_resp_min,
       "finish_ms_response": finish_ms(dev, response)[0], "finish_ms_response_prob": finish_ms(dev, lambda: loop()[0])[0]}
if not baseline_only:
    def draw():
        return hb.hlaPredictDraws(dev, snp, n=N, seed=SEED, verbose=False)

    t_draw, t_draw_min, d = timed(draw)
    equal = (np.array_equal(d.h1, want["h1"]) and np.array_equal(d.h2, want["h2"])
             and np.array_equal(d.prob, want["prob"], equal_nan=True)
             and np.array_equal(d.matching, full.matching, equal_nan=True))
    assert equal, f"{shape}: the device's draws differ from the host sampling"
    res.update({"draws_s": t_draw, "draws_min_s": t_draw_min, "draws_bytes_per_sample": N * 20 + 8,
                "speedup_over_loop": t_loop / t_draw, "over_response": t_draw / t_resp,
                "finish_ms_draws": finish_ms(dev, draw)[0], "draws_equal": bool(equal)})
hb.hlaClose(dev)
print(json.dumps(res))
