#!/usr/bin/env python3
"""hlaPredictGroups against what it replaces, on one device, host arrays in and out: the benchmark's HLA-B shape
(100 classifiers, 10,000 samples), 100 random partitions of the 50 alleles into 2-6 groups, with group dosages.  Each
figure is the median of repeated calls after warm-up calls:
  groups    hlaPredictGroups(dosage=True)
  collapse  hlaPredict(type="response+prob") followed by the host collapse in its fastest honest form: per partition one
            product of the posterior matrix with the one-hot cell -> bin matrix (and one with the cell -> group weights for
            the dosages), then an arg-max over the bins.  BLAS adds in its own order, so this route is close to, not equal
            to, the contract.
  response  hlaPredict(type="response"): the floor -- what the extra finish is paid on top of
plus the event time of the finish kernels of one call of each from the model's timing API.  The exact reference
(tests/groups_reference.py) is run once on the downloaded posterior matrix and must EQUAL the device's arrays; how often the
collapse route's calls and probabilities agree with them is reported.  Prints one JSON line.

Usage: python tools/groups_bench.py [samples [repeats [partitions]]]"""
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
from groups_reference import cell_pairs, groups_from_postprob      # noqa: E402

args = sys.argv[1:]
n_samp = int(args[0]) if len(args) > 0 else 10_000
reps = int(args[1]) if len(args) > 1 else 9
Q = int(args[2]) if len(args) > 2 else 100
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
rng = np.random.default_rng(2025)
group_of = np.stack([rng.integers(0, int(rng.integers(2, 7)), n_hla) for _ in range(Q)]).astype(np.int32)
grp = hb.HlaAlleleGroups.from_matrix(model.hla_allele, group_of)

# the host collapse's matrices, made once (not timed): cell -> bin one-hot and cell -> group weights per partition
h1, h2 = cell_pairs(n_hla)
onehot, weight, pair = [], [], []
for m in group_of.astype(np.int64):
    g = int(m.max()) + 1
    a, b = np.minimum(m[h1], m[h2]), np.maximum(m[h1], m[h2])
    oh = np.zeros((len(h1), g * (g + 1) // 2))
    oh[np.arange(len(h1)), b + a * (2 * g - a - 1) // 2] = 1.0
    w = np.zeros((len(h1), g))
    np.add.at(w, (np.arange(len(h1)), a), 1.0)
    np.add.at(w, (np.arange(len(h1)), b), 1.0)
    onehot.append(oh); weight.append(w); pair.append(np.triu_indices(g))


def collapse():
    r = hb.hlaPredict(dev, snp, type="response+prob", verbose=False)
    pp = r.postprob.T                                 # [n_samp, n_cell], a view
    g1 = np.empty((n_samp, Q), np.int32); g2 = np.empty((n_samp, Q), np.int32); pr = np.empty((n_samp, Q))
    ds = []
    for q in range(Q):
        B = pp @ onehot[q]
        with np.errstate(invalid="ignore"):
            k = np.argmax(np.where(B > 0, B, -np.inf), axis=1)
        best = B[np.arange(n_samp), k]
        ok = best > 0
        g1[:, q] = np.where(ok, pair[q][0][k], hb.NA_INTEGER); g2[:, q] = np.where(ok, pair[q][1][k], hb.NA_INTEGER)
        pr[:, q] = np.where(ok, best, 0.0)
        ds.append(pp @ weight[q])
    return r, g1, g2, pr, np.concatenate(ds, axis=1)


def response():
    return hb.hlaPredict(dev, snp, type="response", verbose=False)


def group_calls():
    return hb.hlaPredictGroups(dev, snp, grp, dosage=True, verbose=False)


t_col, t_col_min, (full, c1, c2, cp, cd) = timed(collapse)
t_resp, t_resp_min, _ = timed(response)
t_grp, t_grp_min, r = timed(group_calls)
want = groups_from_postprob(np.ascontiguousarray(full.postprob.T), n_hla, group_of)
equal = (np.array_equal(r.g1, want["g1"]) and np.array_equal(r.g2, want["g2"]) and np.array_equal(r.prob, want["prob"], equal_nan=True)
         and np.array_equal(r.dosage, want["dosage"], equal_nan=True) and np.array_equal(r.matching, full.matching, equal_nan=True))
assert equal, f"{shape}: the device's group calls differ from the exact reference"
same = (c1 == r.g1) & (c2 == r.g2)
with np.errstate(invalid="ignore"):
    close = np.abs(cp - r.prob) <= 1e-12 * np.maximum(r.prob, 1e-300)
res = {"shape": shape, "n_samp": n_samp, "n_part": Q, "n_level": grp.n_level, "reps": reps, "warmup": WARM,
       "n_classifier": len(model.classifiers), "n_cell": model.n_cell, "postprob_bytes_per_sample": 8 * model.n_cell,
       "groups_bytes_per_sample": Q * 16 + 8 + 8 * grp.n_level,
       "groups_s": t_grp, "groups_min_s": t_grp_min, "collapse_s": t_col, "collapse_min_s": t_col_min,
       "response_s": t_resp, "response_min_s": t_resp_min, "speedup_over_collapse": t_col / t_grp, "over_response": t_grp / t_resp,
       "finish_ms_groups": finish_ms(dev, group_calls)[0], "finish_ms_response": finish_ms(dev, response)[0],
       "finish_ms_response_prob": finish_ms(dev, lambda: hb.hlaPredict(dev, snp, type="response+prob", verbose=False))[0],
       "groups_equal_reference": bool(equal), "collapse_calls_same": float(same.mean()), "collapse_prob_within_1e-12": float(close.mean())}
hb.hlaClose(dev)
print(json.dumps(res))
