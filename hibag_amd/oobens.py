"""``hlaOutOfBagEnsemble``: the out-of-bag estimate of the ENSEMBLE -- every training sample typed by the classifiers whose
bootstrap did not draw it (``samp.num == 0``), the way ``hlaPredict`` types a new sample with the whole model.

``hlaOutOfBag`` (the reference's estimate) averages the accuracies of the single classifiers; this is the estimate bagging
users expect beside it: one prediction per training sample, with ``prob`` and ``matching``, from which a ``call_threshold``
can be chosen on the training data alone.  Sample s gets exactly what ``hlaPredict`` returns for it from the model made
of its out-of-bag classifiers (in model order, with that sub-model's own SNP weights) -- from ONE device call
(:meth:`HlaAttrBagClass.predict_masked`) instead of one sub-model per sample.

The reference has no counterpart; argument checks, the sample / SNP mapping and its errors are ``hlaOutOfBag``'s."""

from __future__ import annotations

import warnings
from typing import Dict, Union

import numpy as np

from .evaluate import hlaCompareAllele
from .hibag import _TYPES, _VOTES, HlaAlleleClass, HlaAttrBagClass, _model_pair_names, _pair_names, hlaModelFromObj
from .model import HlaAttrBagObj, HlaSNPGeno
from .oob import training_cohort

_ENSEMBLE_TYPES = tuple(t for t in _TYPES if t != "prob")      # (the comparison needs the calls)


def out_of_bag_mask(samp_num) -> np.ndarray:
    """``use`` of :meth:`HlaAttrBagClass.predict_masked` from bootstrap counts [n_classifier, n_samp]: uint8, 1 where the
    classifier did not draw the sample."""
    return np.ascontiguousarray(np.asarray(samp_num) == 0, np.uint8)


def hlaOutOfBagEnsemble(model: Union[HlaAttrBagObj, HlaAttrBagClass], hla: HlaAlleleClass, snp: HlaSNPGeno,
                        call_threshold: float = float("nan"), vote: str = "prob", type: str = "response",
                        verbose: bool = True) -> Dict:
    """Ensemble out-of-bag typing of the model's training samples.  Returns a dict:

    ``pred``       :class:`HlaAlleleClass` over ``model.sample_id`` with ``prob`` and ``matching``, and per ``type``
                   (``"response"``, ``"response+dosage"``, ``"response+prob"``) ``dosage`` / ``postprob`` as ``hlaPredict`` lays them out
    ``n_oob``      int32 [n_samp]: out-of-bag classifiers per sample
    ``never_oob``  ids of the samples every classifier drew: not predicted (call NA), left out of the comparison
    ``overall``, ``confusion``, ``confusion_rows``, ``confusion_cols``, ``detail``
                   ``hlaCompareAllele(hla, pred, allele_limit=model, call_threshold=call_threshold, full=True)``
    """
    if not isinstance(model, (HlaAttrBagObj, HlaAttrBagClass)):
        raise TypeError('inherits(model, "hlaAttrBagObj") | inherits(model, "hlaAttrBagClass") is not TRUE')
    if not isinstance(hla, HlaAlleleClass):
        raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
    if not isinstance(snp, HlaSNPGeno):
        raise TypeError('inherits(snp, "hlaSNPGenoClass") is not TRUE')
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    if type not in _ENSEMBLE_TYPES:
        raise ValueError("'arg' should be one of " + ", ".join(f'"{t}"' for t in _ENSEMBLE_TYPES))
    obj = model.obj if isinstance(model, HlaAttrBagClass) else model
    if verbose:
        print(f"HIBAG model for {obj.hla_locus}: {len(obj.classifiers)} individual classifiers, "
              f"{obj.n_snp} SNPs, {obj.n_hla} unique HLA alleles")

    geno, samp_num = training_cohort(obj, hla, snp, every_classifier=False)
    use = out_of_bag_mask(samp_num)
    n_oob = use.sum(axis=0, dtype=np.int32)
    want_dosage, want_prob = type == "response+dosage", type == "response+prob"

    dev = model if isinstance(model, HlaAttrBagClass) else hlaModelFromObj(obj)
    try:
        rv = dev.predict_masked(geno, use, vote_method=_VOTES.index(vote) + 1, want_dosage=want_dosage, want_prob=want_prob)
        pair_names = (_model_pair_names(dev) if dev is model else _pair_names(obj.hla_allele)) if want_prob else []
    finally:
        if dev is not model:
            dev.close()

    ids = list(obj.sample_id)
    pred = HlaAlleleClass(locus=obj.hla_locus, sample_id=ids, h1=rv["h1"], h2=rv["h2"], levels=obj.hla_allele,
                          prob=rv["prob"], matching=rv["matching"], assembly=getattr(obj, "assembly", None) or "unknown",
                          dosage=rv["dosage"].T if want_dosage else None, postprob=rv["postprob"].T if want_prob else None,
                          pair_names=pair_names)
    seen = np.flatnonzero(n_oob > 0)
    never = [ids[k] for k in np.flatnonzero(n_oob == 0)]
    if never:
        warnings.warn(f"{len(never)} training sample{'s are' if len(never) > 1 else ' is'} in-bag in every classifier: "
                      "not predicted, and left out of the comparison.")
    scored = pred if not never else HlaAlleleClass(locus=obj.hla_locus, sample_id=[ids[k] for k in seen], h1=rv["h1"][seen],
                                                   h2=rv["h2"][seen], levels=obj.hla_allele, prob=rv["prob"][seen],
                                                   matching=rv["matching"][seen])
    pam = hlaCompareAllele(hla, scored, allele_limit=obj, call_threshold=call_threshold, full=True)
    if verbose:
        o = pam["overall"]
        print(f"Out-of-bag ensemble: {len(seen)} samples, {int(n_oob[seen].min()) if len(seen) else 0}-"
              f"{int(n_oob.max()) if len(n_oob) else 0} out-of-bag classifiers each, accuracy {100 * o['acc.haplo']:.2f}%")
    return {"pred": pred, "n_oob": n_oob, "never_oob": never, "overall": pam["overall"], "confusion": pam["confusion"],
            "confusion_rows": pam["confusion_rows"], "confusion_cols": pam["confusion_cols"], "detail": pam["detail"]}


__all__ = ["hlaOutOfBagEnsemble", "out_of_bag_mask"]
