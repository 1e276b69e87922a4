"""The R-level helpers the reference's own test script is written with (``tests/runTests.R``):
``hlaSplitAllele`` (``R/DataUtilities.R:1688-1726``), ``hlaFlankingSNP`` (``:1732-1780``),
``hlaGenoSubset`` / ``hlaAlleleSubset`` (``:304-353``, ``:1249-1280``) and the ``overall`` block of
``hlaCompareAllele`` (``:1330-1560``).  Host-side bookkeeping around ``hlaAttrBagging`` and
``hlaPredict``; random draws follow R's ``sample()`` so that ``set_seed(100)`` gives R's split."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from .bed import hlaLociInfo
from .hibag import HlaAlleleClass
from .model import HlaSNPGeno
from .train import RRandom, _R, hlaUniqueAllele


def _unif_index(rng: RRandom, dn: int, sample_kind: str) -> int:
    """``R_unif_index`` (R ``src/main/RNG.c``): "Rounding" is R < 3.6.0's ``floor(dn * unif_rand())``,
    "Rejection" the current default (16-bit chunks, rejection above dn)."""
    if sample_kind == "Rounding":
        return int(math.floor(dn * rng.unif_rand()))
    if dn <= 0:
        return 0
    bits = int(math.ceil(math.log2(dn)))
    while True:
        v = 0
        for _ in range(0, bits + 1, 16):
            v = 65536 * v + int(math.floor(rng.unif_rand() * 65536))
        v &= (1 << bits) - 1
        if v < dn:
            return v


def r_sample(x: Sequence, size: int, rng: Optional[RRandom] = None, sample_kind: str = "Rejection") -> List:
    """``sample(x, size)`` without replacement (``do_sample``, R ``src/main/unique.c`` / ``random.c``)."""
    rng = _R if rng is None else rng
    n = len(x)
    idx = list(range(n))
    out = []
    for _ in range(size):
        j = _unif_index(rng, n, sample_kind)
        out.append(x[idx[j]])
        n -= 1
        idx[j] = idx[n]
    return out


def hlaAlleleSubset(hla: HlaAlleleClass, samp_sel: Sequence[int]) -> HlaAlleleClass:
    ix = list(samp_sel)
    pick = lambda v: None if v is None else np.asarray(v)[ix]      # noqa: E731
    return HlaAlleleClass(locus=hla.locus, sample_id=[hla.sample_id[i] for i in ix], allele1=[hla.allele1[i] for i in ix],
                          allele2=[hla.allele2[i] for i in ix], prob=pick(hla.prob), matching=pick(hla.matching),
                          assembly=hla.assembly)


def hlaSplitAllele(HLA: HlaAlleleClass, train_prop: float = 0.5, rng: Optional[RRandom] = None,
                   sample_kind: str = "Rejection") -> Dict[str, HlaAlleleClass]:
    """``hlaSplitAllele``: repeatedly take the rarest allele, send ``ceiling(n * train.prop)`` of its carriers
    to the training set, drop all its carriers, until no sample is left."""
    ids = [str(s) for s in HLA.sample_id]
    left = list(range(len(ids)))
    train: List[str] = []
    while left:
        a = [HLA.allele1[i] for i in left] + [HLA.allele2[i] for i in left]
        hua = hlaUniqueAllele(a)
        count = {h: 0 for h in hua}
        for v in a:
            if v is not None:
                count[v] += 1
        allele = min(hua, key=lambda h: count[h])          # order(count)[1]: stable, first minimum
        carriers = [i for i in left if HLA.allele1[i] == allele or HLA.allele2[i] == allele]
        n_train = int(math.ceil(len(carriers) * train_prop))
        train.extend(r_sample([ids[i] for i in carriers], n_train, rng, sample_kind))
        gone = set(carriers)
        left = [i for i in left if i not in gone]
    train.sort()                                             # train.set[order(train.set)] (C-locale order for these ids)
    pos = {s: i for i, s in enumerate(ids)}
    tset = set(train)
    return {"training": hlaAlleleSubset(HLA, [pos[s] for s in train]),
            "validation": hlaAlleleSubset(HLA, [i for i, s in enumerate(ids) if s not in tset])}


def hlaFlankingSNP(snp_id: Sequence, position: Sequence[float], locus: str, flank_bp: int = 500000,
                   assembly: str = "auto") -> List:
    info = hlaLociInfo(assembly)
    if info is None or locus not in info:
        raise ValueError("'locus' should be one of " + ", ".join(info or []))
    _, start, end = info[locus]
    if start is None or end is None:
        raise ValueError("The position information is not available!")
    pos = np.asarray(position, np.float64)
    keep = (start - flank_bp <= pos) & (pos <= end + flank_bp)
    return [s for s, k in zip(snp_id, keep) if k]


def hlaGenoSubset(geno: HlaSNPGeno, samp_sel: Optional[Sequence[int]] = None, snp_sel: Optional[Sequence[int]] = None) -> HlaSNPGeno:
    si = list(range(len(geno.sample_id))) if samp_sel is None else list(samp_sel)
    ki = list(range(len(geno.snp_id))) if snp_sel is None else list(snp_sel)
    return HlaSNPGeno(genotype=np.ascontiguousarray(np.asarray(geno.genotype)[np.ix_(ki, si)]),
                      sample_id=[geno.sample_id[i] for i in si], snp_id=[geno.snp_id[i] for i in ki],
                      snp_position=None if geno.snp_position is None else np.asarray(geno.snp_position)[ki],
                      snp_allele=[geno.snp_allele[i] for i in ki], assembly=geno.assembly)


def hlaCompareAllele(TrueHLA: HlaAlleleClass, PredHLA: HlaAlleleClass, allele_limit=None,
                     call_threshold: float = float("nan"), *, full: bool = False) -> Dict:
    """The ``overall`` row of ``hlaCompareAllele``: samples common to both objects whose true alleles are
    within ``allele_limit`` (a model or a list of alleles); a call counts if its probability reaches
    ``call_threshold``.  ``full=True``: R's whole result, ``{"overall", "confusion", "detail"}``
    (:func:`compare_full`)."""
    if full:
        return compare_full(TrueHLA, PredHLA, allele_limit, call_threshold)
    pred = {s: i for i, s in enumerate(PredHLA.sample_id)}
    rows = [(i, pred[s]) for i, s in enumerate(TrueHLA.sample_id) if s in pred]
    # R/DataUtilities.R:1376-1380: samples with an NA in the true OR the predicted pair are left out first
    rows = [(i, j) for i, j in rows if TrueHLA.allele1[i] is not None and TrueHLA.allele2[i] is not None
            and PredHLA.allele1[j] is not None and PredHLA.allele2[j] is not None]
    if allele_limit is not None:
        allowed = set(getattr(allele_limit, "hla_allele", allele_limit))
        rows = [(i, j) for i, j in rows if TrueHLA.allele1[i] in allowed and TrueHLA.allele2[i] in allowed]
    n = len(rows)
    cnt_ind = cnt_haplo = cnt_call = 0
    for i, j in rows:
        if math.isfinite(call_threshold) and PredHLA.prob is not None and not (PredHLA.prob[j] >= call_threshold):
            continue
        cnt_call += 1
        s = [TrueHLA.allele1[i], TrueHLA.allele2[i]]
        p = [PredHLA.allele1[j], PredHLA.allele2[j]]
        if (s[0] == p[0] and s[1] == p[1]) or (s[1] == p[0] and s[0] == p[1]):
            cnt_ind += 1
        if s[0] == p[0] or s[0] == p[1]:
            p[0 if s[0] == p[0] else 1] = ""
            cnt_haplo += 1
        if s[1] == p[0] or s[1] == p[1]:
            cnt_haplo += 1
    return {"total.num.ind": n, "crt.num.ind": cnt_ind, "crt.num.haplo": cnt_haplo,
            "acc.ind": cnt_ind / cnt_call if cnt_call else float("nan"),
            "acc.haplo": 0.5 * cnt_haplo / cnt_call if cnt_call else float("nan"),
            "call.threshold": 0.0 if not math.isfinite(call_threshold) else call_threshold,
            "n.call": cnt_call, "call.rate": cnt_call / n if n else float("nan")}


def confusion_em(m: int, init: np.ndarray, wrong: Sequence[Sequence[int]], n_iter: int = 100) -> np.ndarray:
    """``HIBAG_Confusion`` (``src/HIBAG.cpp:999-1060``): the double miscalls -- both true alleles missed -- split over
    the (true, predicted) cells by 100 EM iterations, in the reference's order of operations.  ``init`` is the
    (m+1) x m confusion matrix (rows predicted, columns true); ``wrong`` lists (t1, t2, p1, p2) row / column indices.
    ``n_iter``: the reference's 100 (others for tests of the first steps)."""
    init = np.asarray(init, np.float64)
    out = init.copy()
    for t1, t2, p1, p2 in wrong:
        out[p1, t1] += 0.5
        out[p2, t1] += 0.5
        out[p1, t2] += 0.5
        out[p2, t2] += 0.5
    for _ in range(n_iter):
        tmp = out
        out = init.copy()
        for t1, t2, p1, p2 in wrong:
            for t in (t1, t2):
                f1, f2 = float(tmp[p1, t]), float(tmp[p2, t])
                s = 1.0 / (f1 + f2)
                out[p1, t] += f1 * s
                out[p2, t] += f2 * s
    return out


def miscall(confusion: np.ndarray, rows: Sequence[str]):
    """The ``miscall`` / ``miscall.prop`` columns (``R/DataUtilities.R:1615-1620``, ``R/HIBAG.R:1377-1380``): per true
    allele the most frequent wrong call (first maximum; None where none) and its share of the wrong calls."""
    rv = np.array(confusion, np.float64)
    m = rv.shape[1]
    rv[np.arange(m), np.arange(m)] = 0.0
    mx = rv.max(axis=0) if m else np.zeros(0)
    idx = rv.argmax(axis=0) if m else np.zeros(0, int)
    names = [None if not (mx[j] > 0) else rows[idx[j]] for j in range(m)]
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = mx / rv.sum(axis=0)
    return names, prop


def compare_full(TrueHLA: HlaAlleleClass, PredHLA: HlaAlleleClass, allele_limit=None,
                 call_threshold: float = float("nan")) -> Dict:
    """``hlaCompareAllele``'s whole result (``R/DataUtilities.R:1328-1622``, default ``match.threshold`` and
    ``max.resolution``): ``overall`` (the dict of ``full=False``), ``confusion`` -- float [(m+1), m], rows the predicted
    alleles plus ``"..."`` (``confusion_rows``), columns the true ones (``confusion_cols``), double miscalls split by
    :func:`confusion_em`, rounded like R's ``round(v, 2)`` -- and ``detail``, a dict of columns."""
    overall = hlaCompareAllele(TrueHLA, PredHLA, allele_limit, call_threshold)
    pred = {s: i for i, s in enumerate(PredHLA.sample_id)}
    rows = [(i, pred[s]) for i, s in enumerate(TrueHLA.sample_id) if s in pred]
    rows = [(i, j) for i, j in rows if TrueHLA.allele1[i] is not None and TrueHLA.allele2[i] is not None
            and PredHLA.allele1[j] is not None and PredHLA.allele2[j] is not None]
    train_freq, train_num = None, float("nan")
    if allele_limit is None:
        allele = hlaUniqueAllele([TrueHLA.allele1[i] for i, _ in rows] + [TrueHLA.allele2[i] for i, _ in rows])
    elif hasattr(allele_limit, "hla_allele"):
        allele = hlaUniqueAllele(list(allele_limit.hla_allele))
        train_freq = None if allele_limit.hla_freq is None else np.asarray(allele_limit.hla_freq, np.float64)
        train_num = float(allele_limit.n_samp)
    else:
        allele = hlaUniqueAllele([str(a) for a in allele_limit])
    pos = {a: k for k, a in enumerate(allele)}
    rows = [(i, j) for i, j in rows if TrueHLA.allele1[i] in pos and TrueHLA.allele2[i] in pos]
    m, n = len(allele), len(rows)
    fn = lambda x: pos.get(x, m)                              # noqa: E731  (the row "...")
    true_num, true_all, pred_num = np.zeros(m), np.zeros(m), np.zeros(m + 1)
    conf = np.zeros((m + 1, m))
    wrong = []
    cnt_call = 0
    thr = math.isfinite(call_threshold) and PredHLA.prob is not None
    for i, j in rows:
        t1, t2 = TrueHLA.allele1[i], TrueHLA.allele2[i]
        q1, q2 = PredHLA.allele1[j], PredHLA.allele2[j]
        true_all[pos[t1]] += 1
        true_all[pos[t2]] += 1
        if thr and not (PredHLA.prob[j] >= call_threshold):
            continue
        true_num[pos[t1]] += 1
        true_num[pos[t2]] += 1
        pred_num[fn(q1)] += 1
        pred_num[fn(q2)] += 1
        p = [q1, q2]
        hnum = 0
        if t1 == p[0] or t1 == p[1]:
            p[0 if t1 == p[0] else 1] = ""
            conf[pos[t1], pos[t1]] += 1
            hnum += 1
        if t2 == p[0] or t2 == p[1]:
            conf[pos[t2], pos[t2]] += 1
            hnum += 1
        if hnum == 1:                                         # the one missed true allele against the one wrong call
            if t1 == q1 or t1 == q2:
                conf[fn(q2 if t1 == q1 else q1), pos[t2]] += 1
            else:
                conf[fn(q2 if t2 == q1 else q1), pos[t1]] += 1
        elif hnum == 0:
            wrong.append((pos[t1], pos[t2], fn(q1), fn(q2)))
        cnt_call += 1
    conf = np.vectorize(lambda v: round(float(v), 2), otypes=[np.float64])(confusion_em(m, conf, wrong)) if m else conf
    detail: Dict[str, object] = {"allele": list(allele)}
    if train_freq is not None:
        detail["train.num"] = 2 * train_freq * train_num
        detail["train.freq"] = train_freq
    diag = conf[np.arange(m), np.arange(m)]
    row_sum = conf.sum(axis=1)[:m]
    with np.errstate(divide="ignore", invalid="ignore"):
        detail["valid.num"] = true_all
        detail["valid.freq"] = true_all / true_all.sum()
        call_rate = true_num / true_all
        sens = diag / true_num
        spec = 1 - (pred_num[:m] - diag) / (2 * cnt_call - true_num)
        acc = (sens * true_num + spec * (2 * cnt_call - true_num)) / (2 * cnt_call)
        ppv = diag / row_sum
        npv = 1 - (true_num - diag) / (2 * n - row_sum)
    call_rate[~np.isfinite(call_rate)] = 0.0
    none = call_rate <= 0
    for v in (sens, spec, ppv, npv, acc):
        v[none] = np.nan
    detail.update({"call.rate": call_rate, "accuracy": acc, "sensitivity": sens, "specificity": spec, "ppv": ppv, "npv": npv})
    names = list(allele) + ["..."]
    detail["miscall"], detail["miscall.prop"] = miscall(conf, names)
    return {"overall": overall, "confusion": conf, "confusion_rows": names, "confusion_cols": list(allele), "detail": detail}
