#!/usr/bin/env python3
"""hlaSNPImportance end to end against two baselines that use nothing but the API the library had before it.  Workload: the
synthetic HLA-B model (100 classifiers) with 1,000 training samples and a seeded bootstrap (the setup of
tools/oobens_bench.py).  Prints one JSON line.

  1. the hand loop: per (classifier, SNP of that classifier) a one-classifier hlaModelFromObj -> hlaPredict of its
     out-of-bag samples with that SNP's row NA -> hlaClose.  Timed on the first `loop_variants` variants and scaled to all
     of them (the output says so); on those variants the new entry's raw predictions are asserted bit-equal.
  2. the strongest thing the older API allows: ONE predict_oob call on a host-built virtual cohort -- a copy of the cohort
     per SNP in use with that SNP's column NA, samp_num nonzero for the classifiers that do not hold it -- plus one
     predict_oob call for the base rows and a numpy tally; its tallies are asserted equal to the new entry's.

Usage: python tools/importance_bench.py [n_samp] [loop_variants] [repeats] [--baselines-only]
--baselines-only: the two baselines alone (what a build of the library without hibag_hip_oob_knock, selected with
HIBAG_HIP_LIBRARY, can run)."""
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hibag_amd as hb                      # noqa: E402
from hibag_amd import NA_INTEGER, synth      # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
baselines_only = "--baselines-only" in sys.argv
n_samp = int(args[0]) if len(args) > 0 else 1000
n_loop = int(args[1]) if len(args) > 1 else 100
reps = int(args[2]) if len(args) > 2 else 3
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
truth = np.ascontiguousarray(truth, np.int32)
samp_num = np.stack([c.samp_num for c in obj.classifiers])
C = len(obj.classifiers)
G_model = np.ascontiguousarray(np.asarray(snp.genotype).T, np.int32)                     # [n_samp, n_snp]
variants = [(c, int(s)) for c, k in enumerate(obj.classifiers) for s in k.snpidx]
n_loop = min(n_loop, len(variants))
used = sorted({s for _, s in variants})


def hand_loop():
    out = []
    for c, s in variants[:n_loop]:
        cls = obj.classifiers[c]
        oob = np.flatnonzero(cls.samp_num == 0)
        g = np.ascontiguousarray(G_model[oob].T)                                          # [n_snp, n_oob], R's argument
        g[s, :] = NA_INTEGER
        m = hb.hlaModelFromObj(dataclasses.replace(obj, classifiers=[cls]))
        v = hb.hlaPredict(m, g, type="response", verbose=False)
        hb.hlaClose(m)
        out.append((oob, np.asarray(v.h1), np.asarray(v.h2), np.asarray(v.prob)))
    return out


def tally_rows(h1, h2, prob, b1, b2, t, thr=float("nan")):
    """The five counts of DESIGN.md section 21 for one row's counted lanes (numpy restatement)."""
    called = (h1 != NA_INTEGER) & (h2 != NA_INTEGER)
    if np.isfinite(thr):
        called &= prob >= thr
    a1 = t[:, 0] == h1
    b = ~a1 & (t[:, 0] == h2)
    second = (~a1 & (t[:, 1] == h1)) | (~b & (t[:, 1] == h2))
    both = (a1 & (t[:, 1] == h2)) | ((t[:, 1] == h1) & (t[:, 0] == h2))
    changed = 0 if b1 is None else int(np.count_nonzero((h1 != b1) | (h2 != b2)))
    return [len(h1), int(called.sum()), int((called & both).sum()), int((called & (a1 | b)).sum() + (called & second).sum()), changed]


def virtual_cohort(model):
    """Baseline 2: every (classifier, SNP) prediction from ONE predict_oob call on n_samp x len(used) virtual samples."""
    base = model.predict_oob(G_model, samp_num)
    Gv = np.tile(G_model, (len(used), 1))
    sv = np.ones((C, n_samp * len(used)), np.int32)
    for i, s in enumerate(used):
        Gv[i * n_samp:(i + 1) * n_samp, s] = NA_INTEGER
    at = {s: i for i, s in enumerate(used)}
    for c, s in variants:
        sv[c, at[s] * n_samp:(at[s] + 1) * n_samp] = samp_num[c]
    out = model.predict_oob(Gv, sv)
    known = np.all(truth != NA_INTEGER, axis=1)
    tally = np.zeros((len(variants) + C, 5), np.int64)
    for c in range(C):
        k = np.flatnonzero((samp_num[c] == 0) & known)
        tally[len(variants) + c] = tally_rows(base["h1"][c, k], base["h2"][c, k], base["prob"][c, k], None, None, truth[k])
    for v, (c, s) in enumerate(variants):
        k = np.flatnonzero((samp_num[c] == 0) & known)
        kv = at[s] * n_samp + k
        tally[v] = tally_rows(out["h1"][c, kv], out["h2"][c, kv], out["prob"][c, kv], base["h1"][c, k], base["h2"][c, k], truth[k])
    return tally


def best(f, n=reps):
    f()                                                   # (warm-up)
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return min(ts), out


model = hb.hlaModelFromObj(obj)
t_loop, loop = best(hand_loop)
t_virt, virt = best(lambda: virtual_cohort(model))
line = {"n_classifier": C, "n_samp": n_samp, "n_variant": len(variants), "snps_in_use": len(used),
        "oob_lanes": int(sum(int((samp_num[c] == 0).sum()) for c, _ in variants)),
        "loop_variants": n_loop, "hand_loop_measured_s": t_loop, "hand_loop_scaled_s": t_loop * len(variants) / n_loop,
        "note": f"hand loop timed on the first {n_loop} variants, scaled by {len(variants)}/{n_loop}",
        "virtual_cohort_s": t_virt, "virtual_cohort_samples": n_samp * len(used),
        "virtual_cohort_upload_bytes": int(n_samp * len(used) * obj.n_snp * 4)}
if not baselines_only:
    t_imp, imp = best(lambda: hb.hlaSNPImportance(model, hla, snp, detail=True, verbose=False))
    t_call, raw = best(lambda: model.predict_oob_knock(G_model, samp_num, truth))
    raw = model.predict_oob_knock(G_model, samp_num, truth, raw=True)
    for v, (oob, h1, h2, prob) in enumerate(loop):
        for name, a, b in (("h1", raw["h1"][v, oob], h1), ("h2", raw["h2"][v, oob], h2)):
            assert np.array_equal(a, b), f"predict_oob_knock and the hand loop differ in '{name}' of variant {v}"
        assert np.array_equal(np.ascontiguousarray(raw["prob"][v, oob]).view(np.uint64), np.ascontiguousarray(prob, np.float64).view(np.uint64)), \
            f"predict_oob_knock and the hand loop differ in 'prob' of variant {v}"
    assert np.array_equal(raw["tally"], virt), "predict_oob_knock and the virtual cohort's numpy tally differ"
    assert np.array_equal(imp.variant_tally, virt[:len(variants)]) and np.array_equal(imp.base_tally, virt[len(variants):])
    top = [int(s) for s in imp.ranking()[:5]]
    line.update({"hlaSNPImportance_s": t_imp, "predict_oob_knock_call_s": t_call,
                 "speedup_vs_hand_loop": line["hand_loop_scaled_s"] / t_imp, "speedup_vs_virtual_cohort": t_virt / t_imp,
                 "bit_equal_on_loop_variants": True, "tallies_equal_virtual_cohort": True,
                 "top_snps": top, "top_importance": [float(imp.importance[s]) for s in top],
                 "snps_with_positive_importance": int(np.count_nonzero(imp.importance > 0))})
model.close()
print(json.dumps(line))
