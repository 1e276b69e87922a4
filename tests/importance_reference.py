"""The yardstick of hlaSNPImportance, on the oracle alone: per classifier a one-classifier model, per
SNP of that classifier ``oracle.predict`` of its out-of-bag samples with that SNP's column set to NA (as ``oracle_oob`` of
tests/test_oob_host.py does for the base), then the tallies of definition 4 and the summary of definition 5 in plain Python.
Nothing here touches the library."""
import dataclasses
import math

import numpy as np

from hibag_amd import NA_INTEGER

COLS = ("n_ind", "n_call", "crt_ind", "crt_haplo", "n_changed")


def truth_of(model, hla_type_table, locus="A"):
    """int32 [n, 2]: the training samples' true alleles as indices of model.hla_allele; NA in both columns where an
    allele is unknown or not among the model's."""
    tab = {s: (a, b) for s, a, b in zip(hla_type_table["sample.id"], hla_type_table[locus + ".1"], hla_type_table[locus + ".2"])}
    idx = {a: i for i, a in enumerate(model.hla_allele)}
    out = np.full((len(model.sample_id), 2), NA_INTEGER, np.int32)
    for k, s in enumerate(model.sample_id):
        a, b = tab.get(s, (None, None))
        if a in idx and b in idx:
            out[k] = (idx[a], idx[b])
    return out


def samp_num_of(model):
    return np.stack([np.asarray(c.samp_num, np.int32) for c in model.classifiers])


def variants_of(model):
    """(classifier, snp) of every variant, v = snp_off[c] + j."""
    cls = [c for c, k in enumerate(model.classifiers) for _ in k.snpidx]
    snp = [int(s) for k in model.classifiers for s in k.snpidx]
    return np.array(cls, np.int32), np.array(snp, np.int32)


def tally_row(h1, h2, prob, base_h1, base_h2, truth, oob, thr):
    """Definition 4 for one row: hlaCompareAllele's counting (hibag_amd/evaluate.py:125-143) on allele indices."""
    n_ind = n_call = crt_ind = crt_haplo = n_changed = 0
    for i in oob:
        t = [int(truth[i, 0]), int(truth[i, 1])]
        if t[0] == NA_INTEGER or t[1] == NA_INTEGER:
            continue
        n_ind += 1
        if base_h1 is not None and (h1[i] != base_h1[i] or h2[i] != base_h2[i]):
            n_changed += 1
        if h1[i] == NA_INTEGER or h2[i] == NA_INTEGER:           # (hlaCompareAllele leaves a sample without a call out)
            continue
        if math.isfinite(thr) and not (prob[i] >= thr):
            continue
        n_call += 1
        p = [int(h1[i]), int(h2[i])]
        if (t[0] == p[0] and t[1] == p[1]) or (t[1] == p[0] and t[0] == p[1]):
            crt_ind += 1
        if t[0] == p[0] or t[0] == p[1]:
            p[0 if t[0] == p[0] else 1] = None
            crt_haplo += 1
        if t[1] == p[0] or t[1] == p[1]:
            crt_haplo += 1
    return [n_ind, n_call, crt_ind, crt_haplo, n_changed]


def knock_raw(oracle, model, G, avx2=False, n_threads=1):
    """h1, h2, prob [n_variant + C, n]: the variants' rows, then the base rows; NA / 0 in the bag."""
    C, n = len(model.classifiers), G.shape[0]
    vc, vs = variants_of(model)
    nv = len(vc)
    h1 = np.full((nv + C, n), NA_INTEGER, np.int32)
    h2 = np.full((nv + C, n), NA_INTEGER, np.int32)
    prob = np.zeros((nv + C, n))
    v = 0
    for c, cls in enumerate(model.classifiers):
        oob = np.flatnonzero(np.asarray(cls.samp_num) == 0)
        fm = oracle.flatten(dataclasses.replace(model, classifiers=[cls]))
        if len(oob):
            r = oracle.predict(fm, np.ascontiguousarray(G[oob]), 1, want_dosage=False, want_prob=False, avx2=avx2, n_threads=n_threads)
            h1[nv + c, oob], h2[nv + c, oob], prob[nv + c, oob] = r["h1"], r["h2"], r["prob"]
        for s in cls.snpidx:
            if len(oob):
                Gk = np.ascontiguousarray(G[oob])
                Gk[:, int(s)] = NA_INTEGER
                r = oracle.predict(fm, Gk, 1, want_dosage=False, want_prob=False, avx2=avx2, n_threads=n_threads)
                h1[v, oob], h2[v, oob], prob[v, oob] = r["h1"], r["h2"], r["prob"]
            v += 1
    return {"h1": h1, "h2": h2, "prob": prob, "classifier": vc, "snp": vs, "n_variant": nv}


def knock_tally(model, raw, truth, thr=float("nan")):
    """int64 [n_variant + C, 5] from the raw predictions."""
    C = len(model.classifiers)
    nv = raw["n_variant"]
    out = np.zeros((nv + C, 5), np.int64)
    oobs = [np.flatnonzero(np.asarray(c.samp_num) == 0) for c in model.classifiers]
    for c in range(C):
        out[nv + c] = tally_row(raw["h1"][nv + c], raw["h2"][nv + c], raw["prob"][nv + c], None, None, truth, oobs[c], thr)
    for v in range(nv):
        c = int(raw["classifier"][v])
        out[v] = tally_row(raw["h1"][v], raw["h2"][v], raw["prob"][v], raw["h1"][nv + c], raw["h2"][nv + c], truth, oobs[c], thr)
    return out


def summary(model, tally):
    """Definition 5: dict of per-SNP lists (float NaN where undefined), from the integer tallies."""
    S, C = model.n_snp, len(model.classifiers)
    nv = tally.shape[0] - C
    users = [[] for _ in range(S)]                         # (variant, classifier) in model order
    v = 0
    for c, cls in enumerate(model.classifiers):
        for s in cls.snpidx:
            users[int(s)].append((v, c))
            v += 1
    nan = float("nan")
    res = {k: [] for k in ("n_classifier", "n_used", "importance", "acc_base", "acc_drop", "importance_ind", "changed")}
    for s in range(S):
        imp = ab = ad = ind = 0.0
        used = chg = tot = 0
        for v, c in users[s]:
            b, t = [int(x) for x in tally[nv + c]], [int(x) for x in tally[v]]
            chg += t[4]
            tot += t[0]
            if b[1] == 0 or t[1] == 0:
                continue
            used += 1
            a0, a1 = 0.5 * b[3] / b[1], 0.5 * t[3] / t[1]
            imp += a0 - a1
            ab += a0
            ad += a1
            ind += b[2] / b[1] - t[2] / t[1]
        res["n_classifier"].append(len(users[s]))
        res["n_used"].append(used)
        for k, x in (("importance", imp), ("acc_base", ab), ("acc_drop", ad), ("importance_ind", ind)):
            res[k].append(x / used if used else nan)
        res["changed"].append(chg / tot if tot else nan)
    return res


def ranking(importance):
    """SNPs by descending importance, NaN last, ties in SNP order."""
    return sorted(range(len(importance)), key=lambda s: (math.isnan(importance[s]), -importance[s] if not math.isnan(importance[s]) else 0.0, s))


_RAW = {}


def cached_raw(key, oracle, model, G, **kw):
    """knock_raw once per session and `key` (the tests of both files share it; nobody writes to it)."""
    if key not in _RAW:
        raw = knock_raw(oracle, model, G, **kw)
        for k in ("h1", "h2", "prob"):
            raw[k].setflags(write=False)
        _RAW[key] = raw
    return _RAW[key]
