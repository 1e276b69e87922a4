"""``hlaOutOfBag`` (``R/HIBAG.R:1275-1386``): how well a trained model predicts, measured on each classifier's out-of-bag
(OOB) samples -- the training samples its bootstrap did not draw (``samp.num == 0``).

The reference loops over the classifiers: a one-classifier model each, ``hlaPredict`` of its OOB samples,
``hlaCompareAllele``.  Here every classifier's predictions come from ONE batched device call
(:meth:`HlaAttrBagClass.predict_oob`, bit-identical to that loop); what is left on the host is the comparison and the
averaging, on O(classifiers x samples) integers.

Deviation: a classifier without a single OOB sample raises ``ValueError`` naming it (R would fail inside
``hlaPredict``).  ``load_model`` fills a missing ``samp.num`` with ones, so a loaded model without bootstrap counts
reaches that error rather than R's "There is no bootstrap sample index."."""

from __future__ import annotations

from typing import Dict, Union

import numpy as np

from .evaluate import hlaCompareAllele, miscall
from .hibag import HlaAlleleClass, HlaAttrBagClass, hlaModelFromObj
from .model import HlaAttrBagObj, HlaSNPGeno

_DETAIL_AVG = ("call.rate", "accuracy", "sensitivity", "specificity", "ppv", "npv")


def training_cohort(obj: HlaAttrBagObj, hla: HlaAlleleClass, snp: HlaSNPGeno, every_classifier: bool):
    """The model's training samples and SNPs found in ``hla`` and ``snp`` (``R/HIBAG.R:1297-1313``, its errors), and the
    bootstrap counts: ``geno`` int32 [n_samp, n_snp] in ``sample_id`` / ``snp_id`` order of the model and ``samp_num`` int32
    [n_classifier, n_samp].  ``every_classifier``: a classifier without an out-of-bag sample raises (what ``hlaOutOfBag``,
    which evaluates classifier by classifier, cannot do without)."""
    if not obj.sample_id:
        raise ValueError("There is no sample ID in the model.")
    spos = {s: i for i, s in enumerate(snp.sample_id)}
    if any(s not in spos for s in obj.sample_id):
        raise ValueError("Some of sample.id in the model do not exist in SNP genotypes.")
    hpos = {s: i for i, s in enumerate(hla.sample_id)}
    if any(s not in hpos for s in obj.sample_id):
        raise ValueError("Some of sample.id in the model do not exist in HLA types.")
    kpos = {s: i for i, s in enumerate(snp.snp_id)}
    if any(s not in kpos for s in obj.snp_id):
        raise ValueError("Some of snp.id in the model do not exist in SNP genotypes.")
    samp_idx = np.array([spos[s] for s in obj.sample_id], np.int64)
    snp_idx = np.array([kpos[s] for s in obj.snp_id], np.int64)
    geno = np.ascontiguousarray(np.asarray(snp.genotype)[np.ix_(snp_idx, samp_idx)].T, np.int32)     # [n_samp, n_snp]

    nclass = len(obj.classifiers)
    n = len(obj.sample_id)
    samp_num = np.empty((nclass, n), np.int32)
    for i, c in enumerate(obj.classifiers):
        if c.samp_num is None:
            raise ValueError("There is no bootstrap sample index.")
        sn = np.asarray(c.samp_num)
        if sn.shape != (n,):
            raise ValueError(f"classifier {i + 1}: samp.num has {sn.size} entries, the model {n} samples")
        if every_classifier and not np.any(sn == 0):
            raise ValueError(f"classifier {i + 1} has no out-of-bag sample: it cannot be evaluated")
        samp_num[i] = sn
    return geno, samp_num


def hlaOutOfBag(model: Union[HlaAttrBagObj, HlaAttrBagClass], hla: HlaAlleleClass, snp: HlaSNPGeno,
                call_threshold: float = float("nan"), verbose: bool = True) -> Dict:
    """Out-of-bag accuracy of ``model``: R's ``list(overall, confusion, detail)`` averaged over the classifiers.
    ``confusion`` comes with ``confusion_rows`` / ``confusion_cols``, ``detail`` is a dict of columns."""
    if not isinstance(model, (HlaAttrBagObj, HlaAttrBagClass)):
        raise TypeError('inherits(model, "hlaAttrBagObj") | inherits(model, "hlaAttrBagClass") is not TRUE')
    if not isinstance(hla, HlaAlleleClass):
        raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
    if not isinstance(snp, HlaSNPGeno):
        raise TypeError('inherits(snp, "hlaSNPGenoClass") is not TRUE')
    obj = model.obj if isinstance(model, HlaAttrBagClass) else model
    if verbose and isinstance(model, HlaAttrBagClass):
        print(f"HIBAG model for {obj.hla_locus}: {len(obj.classifiers)} individual classifiers, "
              f"{obj.n_snp} SNPs, {obj.n_hla} unique HLA alleles")

    geno, samp_num = training_cohort(obj, hla, snp, every_classifier=True)
    nclass = len(obj.classifiers)

    dev = model if isinstance(model, HlaAttrBagClass) else hlaModelFromObj(obj)
    try:
        out = dev.predict_oob(geno, samp_num)
    finally:
        if dev is not model:
            dev.close()

    # one comparison per classifier, then R's averaging (R/HIBAG.R:1336-1385)
    ids = list(obj.sample_id)
    ans = None
    for i in range(nclass):
        oob = np.flatnonzero(samp_num[i] == 0)
        pred = HlaAlleleClass(locus=obj.hla_locus, sample_id=[ids[k] for k in oob], prob=out["prob"][i, oob],
                              h1=out["h1"][i, oob], h2=out["h2"][i, oob], levels=obj.hla_allele)
        pam = hlaCompareAllele(hla, pred, allele_limit=obj, call_threshold=call_threshold, full=True)
        det = np.array([pam["detail"][k] for k in _DETAIL_AVG], np.float64)
        ok = ~np.isnan(det)
        det[~ok] = 0.0
        if ans is None:
            ans = pam
            # (R keeps the first result's allele / train.num / train.freq, renamed valid.num / valid.freq)
            d = pam["detail"]
            ans["head"] = {"allele": d["allele"], "valid.num": d.get("train.num"), "valid.freq": d.get("train.freq")}
            ans["overall"] = dict(pam["overall"])
            ans["n_detail"] = ok.astype(np.float64)
            ans["det"] = det
        else:
            for k, v in pam["overall"].items():
                ans["overall"][k] = ans["overall"][k] + v
            ans["confusion"] = ans["confusion"] + pam["confusion"]
            ans["n_detail"] = ans["n_detail"] + ok
            ans["det"] = ans["det"] + det
        if verbose:
            print(f"passing the {i + 1}/{nclass} classifiers.")

    overall = {k: v / nclass for k, v in ans["overall"].items()}
    confusion = ans["confusion"] / nclass
    with np.errstate(divide="ignore", invalid="ignore"):
        det = ans["det"] / ans["n_detail"]
    detail = dict(ans["head"])
    detail.update({k: det[j] for j, k in enumerate(_DETAIL_AVG)})
    detail["miscall"], detail["miscall.prop"] = miscall(confusion, ans["confusion_rows"])
    return {"overall": overall, "confusion": confusion, "confusion_rows": ans["confusion_rows"],
            "confusion_cols": ans["confusion_cols"], "detail": detail}


__all__ = ["hlaOutOfBag"]
