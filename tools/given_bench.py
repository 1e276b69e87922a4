#!/usr/bin/env python3
"""hlaPredictGiven against what it replaces, on one device, host arrays in and out: the benchmark's HLA-B shape
(100 classifiers, 10,000 samples), every sample constrained to its true two-digit groups, with dosages.  Each figure is the
median of repeated calls after warm-up calls:
  given     hlaPredictGiven(dosage=True)
  masked    hlaPredict(type="response+prob") followed by the host route in its fastest honest form: the consistency mask
            over the cells from two gathers, one masked arg-max, the support as a row sum and the dosages as one product of
            the masked matrix with the cell -> allele weights.  numpy and BLAS add in their own order, so the support and
            the dosages of this route are close to, not equal to, the contract.
  response  hlaPredict(type="response"): the floor -- what the extra finish is paid on top of
plus the event time of the finish kernels of one call of each from the model's timing API.  The exact reference
(tests/given_reference.py) is run once on the downloaded posterior matrix and must EQUAL the device's arrays; how often the
masked route's calls agree with them is reported.  Prints one JSON line.

Usage: python tools/given_bench.py [samples [repeats]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hibag_amd as hb                              # noqa: E402
from hibag_amd import synth                          # noqa: E402
from given_reference import cell_pairs, conditional, given_from_postprob      # noqa: E402

args = sys.argv[1:]
n_samp = int(args[0]) if len(args) > 0 else 10_000
reps = int(args[1]) if len(args) > 1 else 9
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
G, truth = synth.make_samples(founders, af, n_samp)
snp = np.asfortranarray(G.T)                  # [n.snp, n.samp] in R's memory order: the C side's sample-major matrix, no copy
dev = hb.hlaModelFromObj(model)
n_hla = model.n_hla
names = list(model.hla_allele)
two = hb.hlaAlleleDigit(names, "2-digit")
typed = hb.HlaAlleleClass(locus="B", sample_id=list(range(1, n_samp + 1)), allele1=[two[t] for t in truth[:, 0]],
                          allele2=[two[t] for t in truth[:, 1]])
known = hb.hlaConstraintFromAllele(model, typed)
A, B = known.allowed[:, 0], known.allowed[:, 1]

# the host route's constants, made once (not timed): the alleles of every cell, cell -> allele weights
h1, h2 = cell_pairs(n_hla)
weight = np.zeros((len(h1), n_hla))
np.add.at(weight, (np.arange(len(h1)), h1), 1.0)
np.add.at(weight, (np.arange(len(h1)), h2), 1.0)


def masked():
    r = hb.hlaPredict(dev, snp, type="response+prob", verbose=False)
    pp = r.postprob.T                                 # [n_samp, n_cell], a view
    ok = (A[:, h1] & B[:, h2]) | (B[:, h1] & A[:, h2])
    with np.errstate(invalid="ignore"):
        m = np.where(ok, pp, 0.0)
        k = np.argmax(np.where(m > 0, m, -np.inf), axis=1)
    best = m[np.arange(n_samp), k]
    won = best > 0
    support = m.sum(axis=1)
    dosage = m @ weight
    return (r, np.where(won, h1[k], hb.NA_INTEGER).astype(np.int32), np.where(won, h2[k], hb.NA_INTEGER).astype(np.int32),
            np.where(won, best, 0.0), support, dosage)


def response():
    return hb.hlaPredict(dev, snp, type="response", verbose=False)


def given_calls():
    return hb.hlaPredictGiven(dev, snp, known, dosage=True, verbose=False)


t_msk, t_msk_min, (full, m1, m2, mp, ms, md) = timed(masked)
t_resp, t_resp_min, plain = timed(response)
t_giv, t_giv_min, r = timed(given_calls)
want = given_from_postprob(np.ascontiguousarray(full.postprob.T), n_hla, known.allowed)
cond = conditional(want)
equal = (np.array_equal(r.h1, want["h1"]) and np.array_equal(r.h2, want["h2"]) and np.array_equal(r.prob_joint, want["prob"], equal_nan=True)
         and np.array_equal(r.support, want["support"], equal_nan=True) and np.array_equal(r.prob, cond["prob"], equal_nan=True)
         and np.array_equal(r.dosage, cond["dosage"].T, equal_nan=True) and np.array_equal(r.matching, full.matching, equal_nan=True))
assert equal, f"{shape}: the device's given calls differ from the exact reference"
same = (m1 == r.h1) & (m2 == r.h2)
hit = lambda a, b: float(np.mean((a == truth[:, 0]) & (b == truth[:, 1])))
res = {"shape": shape, "n_samp": n_samp, "reps": reps, "warmup": WARM, "n_classifier": len(model.classifiers),
       "n_cell": model.n_cell, "postprob_bytes_per_sample": 8 * model.n_cell, "given_bytes_per_sample": 24 + 8 + 8 * n_hla,
       "given_s": t_giv, "given_min_s": t_giv_min, "masked_s": t_msk, "masked_min_s": t_msk_min,
       "response_s": t_resp, "response_min_s": t_resp_min, "speedup_over_masked": t_msk / t_giv, "over_response": t_giv / t_resp,
       "finish_ms_given": finish_ms(dev, given_calls)[0], "finish_ms_response": finish_ms(dev, response)[0],
       "finish_ms_response_prob": finish_ms(dev, lambda: hb.hlaPredict(dev, snp, type="response+prob", verbose=False))[0],
       "given_equal_reference": bool(equal), "masked_calls_same": float(same.mean()),
       "calls_changed": int(np.count_nonzero((r.h1 != plain.h1) | (r.h2 != plain.h2))),
       "pair_accuracy_plain": hit(plain.h1, plain.h2), "pair_accuracy_given": hit(r.h1, r.h2)}
hb.hlaClose(dev)
print(json.dumps(res))
