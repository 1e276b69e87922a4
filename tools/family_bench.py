#!/usr/bin/env python3
"""hlaPredictFamily against what it replaces, on one device, host arrays in and out: the benchmark's HLA-B shape
(100 classifiers, 10,000 samples) as 3,333 trios and one founder, parents first, with dosages.  Each figure is the median of
repeated calls after warm-up calls:
  family    hlaPredictFamily(dosage=True)
  weighted  hlaPredict(type="response+prob") followed by the host route in its fastest honest form, vectorised over the
            samples: the parents' dosages as one product of their rows with the cell -> allele weights and their supports as
            row sums, the ratio vectors, the children's weights from four gathers, one arg-max, the support as a row sum and
            the dosages as one product.  numpy and BLAS add in their own order, so this route's values are close to, not
            equal to, the contract.
  response  hlaPredict(type="response"): the floor -- what the extra finish is paid on top of
plus the event time of the finish kernels of one call of each from the model's timing API.  The exact reference
(tests/family_reference.py) is run once on the downloaded posterior matrix and must EQUAL the device's arrays; how often the
host route's calls agree with them is reported.  Prints one JSON line.

Usage: python tools/family_bench.py [trios [repeats]]"""
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
from family_reference import cell_pairs, conditional, family_from_postprob      # noqa: E402

args = sys.argv[1:]
n_fam = int(args[0]) if len(args) > 0 else 3333
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
G, truth, ped = synth.make_family(founders, af, n_fam)
g1, t1 = synth.make_samples(founders, af, 1)
G = np.ascontiguousarray(np.concatenate([G, g1]))
truth = np.concatenate([truth, t1])
ped = np.concatenate([ped, np.full((1, 2), -1, np.int32)])
n_samp = len(G)
snp = np.asfortranarray(G.T)                  # [n.snp, n.samp] in R's memory order: the C side's sample-major matrix, no copy
dev = hb.hlaModelFromObj(model)
n_hla = model.n_hla
q = hb.hlaModelAllelePrior(model)
kids = np.nonzero(ped[:, 0] >= 0)[0]
fa, mo = ped[kids, 0], ped[kids, 1]

# the host route's constants, made once (not timed): the alleles of every cell, cell -> allele weights
h1, h2 = cell_pairs(n_hla)
weight = np.zeros((len(h1), n_hla))
np.add.at(weight, (np.arange(len(h1)), h1), 1.0)
np.add.at(weight, (np.arange(len(h1)), h2), 1.0)


def weighted():
    r = hb.hlaPredict(dev, snp, type="response+prob", verbose=False)
    pp = r.postprob.T                                 # [n_samp, n_cell], a view
    par = np.unique(np.concatenate([fa, mo]))
    D = np.zeros((n_samp, n_hla))
    S = np.zeros(n_samp)
    D[par] = pp[par] @ weight
    S[par] = pp[par].sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        def ratio(p):
            ok = S[p] > 0
            return np.where(ok[:, None], 0.5 * (D[p] / np.where(ok, S[p], 1.0)[:, None]) / q, 1.0)
        rf, rm = ratio(fa), ratio(mo)
        x = pp[kids] * (0.5 * (rf[:, h1] * rm[:, h2] + rf[:, h2] * rm[:, h1]))
        k = np.argmax(np.where(x > 0, x, -np.inf), axis=1)
    best = x[np.arange(len(kids)), k]
    won = best > 0
    c1, c2, prob = r.h1.copy(), r.h2.copy(), r.prob.copy()
    c1[kids] = np.where(won, h1[k], hb.NA_INTEGER)
    c2[kids] = np.where(won, h2[k], hb.NA_INTEGER)
    prob[kids] = np.where(won, best, 0.0)
    support = pp.sum(axis=1)
    support[kids] = x.sum(axis=1)
    dosage = pp @ weight
    dosage[kids] = x @ weight
    return r, c1, c2, prob, support, dosage


def response():
    return hb.hlaPredict(dev, snp, type="response", verbose=False)


def family_calls():
    return hb.hlaPredictFamily(dev, snp, ped, dosage=True, verbose=False)


t_wgt, t_wgt_min, (full, m1, m2, mp, ms, md) = timed(weighted)
t_resp, t_resp_min, plain = timed(response)
t_fam, t_fam_min, r = timed(family_calls)
want = family_from_postprob(np.ascontiguousarray(full.postprob.T), n_hla, ped, q)
cond = conditional(want)
equal = (np.array_equal(r.h1, want["h1"]) and np.array_equal(r.h2, want["h2"]) and np.array_equal(r.prob_joint, want["prob"], equal_nan=True)
         and np.array_equal(r.support, want["support"], equal_nan=True) and np.array_equal(r.prob, cond["prob"], equal_nan=True)
         and np.array_equal(r.dosage, cond["dosage"].T, equal_nan=True) and np.array_equal(r.matching, full.matching, equal_nan=True))
assert equal, f"{shape}: the device's family calls differ from the exact reference"
same = (m1 == r.h1) & (m2 == r.h2)
hit = lambda a, b: float(np.mean((a[kids] == truth[kids, 0]) & (b[kids] == truth[kids, 1])))
mendel = lambda x: hb.hlaMendelCheck(x, ped).n_inconsistent_trios
res = {"shape": shape, "n_samp": n_samp, "n_trio": n_fam, "reps": reps, "warmup": WARM, "n_classifier": len(model.classifiers),
       "n_cell": model.n_cell, "postprob_bytes_per_sample": 8 * model.n_cell, "family_bytes_per_sample": 24 + 8 + 8 * n_hla,
       "family_s": t_fam, "family_min_s": t_fam_min, "weighted_s": t_wgt, "weighted_min_s": t_wgt_min,
       "response_s": t_resp, "response_min_s": t_resp_min, "speedup_over_weighted": t_wgt / t_fam, "over_response": t_fam / t_resp,
       "finish_ms_family": finish_ms(dev, family_calls)[0], "finish_ms_response": finish_ms(dev, response)[0],
       "finish_ms_response_prob": finish_ms(dev, lambda: hb.hlaPredict(dev, snp, type="response+prob", verbose=False))[0],
       "family_equal_reference": bool(equal), "weighted_calls_same": float(same.mean()),
       "children_calls_changed": int(np.count_nonzero((r.h1[kids] != plain.h1[kids]) | (r.h2[kids] != plain.h2[kids]))),
       "child_pair_accuracy_plain": hit(plain.h1, plain.h2), "child_pair_accuracy_family": hit(r.h1, r.h2),
       "inconsistent_trios_plain": mendel(plain), "inconsistent_trios_family": mendel(r)}
hb.hlaClose(dev)
print(json.dumps(res))
