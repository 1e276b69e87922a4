"""``hlaSNPImportance``: which SNPs a bagged model leans on -- Breiman's out-of-bag variable importance with HIBAG's own,
noise-free disturbance.  The reference has no counterpart.

Per classifier c and SNP s of c, c predicts its out-of-bag samples (as ``hlaOutOfBag`` has it predict them: a one-classifier
model, vote "prob") with s set to NA -- a missing SNP is marginalised exactly -- and the haplotype accuracy is compared with
the one c reaches on the same samples with nothing knocked out.  The importance of s is the mean accuracy drop over the
classifiers that hold s.  Every (classifier, SNP) prediction and its comparison with the truth happen in ONE device call
(:meth:`HlaAttrBagClass.predict_oob_knock`), which returns integer tallies; what is left on the host is float64 arithmetic
on O(classifiers x SNPs per classifier) integers.  DESIGN.md section 21 is the definition."""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Union

import numpy as np

from .hibag import NA_INTEGER, HlaAlleleClass, HlaAttrBagClass, hlaModelFromObj
from .model import HlaAttrBagObj, HlaSNPGeno
from .oob import training_cohort

TALLY_COLUMNS = ("n_ind", "n_call", "crt_ind", "crt_haplo", "n_changed")


@dataclass
class HlaSNPImportance:
    """Per model SNP (arrays of length ``n_snp``, model order); a SNP no classifier holds has ``n_classifier`` 0 and NaN
    in the float columns.  ``base_tally`` int64 [n_classifier, 5] and, with ``detail=True``, ``variant_tally`` int64
    [n_variant, 5] with ``variant_classifier`` / ``variant_snp`` hold the counts of :data:`TALLY_COLUMNS`."""
    snp_id: List
    snp_position: Optional[np.ndarray]
    n_classifier: np.ndarray        # users of the SNP
    n_used: np.ndarray              # ... whose pair (base, knock-out) has calls on both sides: what the means are over
    importance: np.ndarray          # mean of acc.haplo(base c) - acc.haplo(c without the SNP)
    acc_base: np.ndarray            # the two means separately
    acc_drop: np.ndarray
    importance_ind: np.ndarray      # the same with acc.ind
    changed: np.ndarray             # share of the counted out-of-bag predictions whose call changes
    base_tally: np.ndarray
    call_threshold: float
    variant_tally: Optional[np.ndarray] = None
    variant_classifier: Optional[np.ndarray] = None
    variant_snp: Optional[np.ndarray] = None

    def ranking(self) -> np.ndarray:
        """SNP indices by descending ``importance``; NaN last, ties in SNP order."""
        key = np.where(np.isnan(self.importance), np.inf, -self.importance)
        return np.argsort(key, kind="stable")


def truth_indices(obj: HlaAttrBagObj, hla: HlaAlleleClass) -> np.ndarray:
    """int32 [n_samp, 2]: the true alleles of the model's training samples as indices of ``obj.hla_allele``; a sample with
    an unknown allele, or one the model does not have, gets NA in both columns (``hlaCompareAllele`` with
    ``allele_limit=obj`` leaves it out)."""
    pos = {s: i for i, s in enumerate(hla.sample_id)}
    idx = {a: i for i, a in enumerate(obj.hla_allele)}
    out = np.full((len(obj.sample_id), 2), NA_INTEGER, np.int32)
    for k, s in enumerate(obj.sample_id):
        i = pos[s]
        a, b = idx.get(hla.allele1[i]), idx.get(hla.allele2[i])
        if a is not None and b is not None:
            out[k] = (a, b)
    return out


def summarise(obj: HlaAttrBagObj, tally: np.ndarray, call_threshold: float, detail: bool) -> HlaSNPImportance:
    """Definition 5 of DESIGN.md section 21 from the tallies [n_variant + n_classifier, 5]: plain float64 sums over a SNP's
    users in model order, divided by the number of pairs used."""
    S, C = obj.n_snp, len(obj.classifiers)
    nv = tally.shape[0] - C
    base = tally[nv:]
    n_cls = np.zeros(S, np.int64)
    n_used = np.zeros(S, np.int64)
    sums = [[0.0] * 4 for _ in range(S)]               # importance, acc_base, acc_drop, importance_ind
    chg = np.zeros((S, 2), np.int64)
    v = 0
    for c, cls in enumerate(obj.classifiers):
        bn, bi, bh = int(base[c, 1]), int(base[c, 2]), int(base[c, 3])
        for s in (int(x) for x in cls.snpidx):
            n_cls[s] += 1
            chg[s, 0] += int(tally[v, 4])
            chg[s, 1] += int(tally[v, 0])
            vn, vi, vh = int(tally[v, 1]), int(tally[v, 2]), int(tally[v, 3])
            if bn > 0 and vn > 0:
                ab, av = 0.5 * bh / bn, 0.5 * vh / vn
                acc = sums[s]
                acc[0] += ab - av
                acc[1] += ab
                acc[2] += av
                acc[3] += bi / bn - vi / vn
                n_used[s] += 1
            v += 1
    cols = np.full((4, S), np.nan)
    changed = np.full(S, np.nan)
    for s in range(S):
        if n_cls[s] == 0:
            continue
        if n_used[s] > 0:
            for k in range(4):
                cols[k, s] = sums[s][k] / int(n_used[s])
        if chg[s, 1] > 0:
            changed[s] = int(chg[s, 0]) / int(chg[s, 1])
    out = HlaSNPImportance(snp_id=list(obj.snp_id), snp_position=None if obj.snp_position is None else np.asarray(obj.snp_position),
                           n_classifier=n_cls, n_used=n_used, importance=cols[0], acc_base=cols[1], acc_drop=cols[2],
                           importance_ind=cols[3], changed=changed, base_tally=np.array(base, np.int64),
                           call_threshold=float(call_threshold))
    if detail:
        out.variant_tally = np.array(tally[:nv], np.int64)
        out.variant_classifier = np.repeat(np.arange(C, dtype=np.int32), [len(c.snpidx) for c in obj.classifiers])
        out.variant_snp = np.concatenate([np.asarray(c.snpidx, np.int32) for c in obj.classifiers] + [np.empty(0, np.int32)])
    return out


def hlaSNPImportance(model: Union[HlaAttrBagObj, HlaAttrBagClass], hla: HlaAlleleClass, snp: HlaSNPGeno,
                     call_threshold: float = float("nan"), detail: bool = False, verbose: bool = True) -> HlaSNPImportance:
    """Out-of-bag knock-out importance of every SNP of ``model``, measured on its training samples found in ``hla`` and
    ``snp`` (matched as ``hlaOutOfBag`` matches them, with its errors).  ``call_threshold`` as for ``hlaCompareAllele``;
    ``detail=True`` keeps the per-(classifier, SNP) tallies."""
    if not isinstance(model, (HlaAttrBagObj, HlaAttrBagClass)):
        raise TypeError('inherits(model, "hlaAttrBagObj") | inherits(model, "hlaAttrBagClass") is not TRUE')
    if not isinstance(hla, HlaAlleleClass):
        raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
    if not isinstance(snp, HlaSNPGeno):
        raise TypeError('inherits(snp, "hlaSNPGenoClass") is not TRUE')
    obj = model.obj if isinstance(model, HlaAttrBagClass) else model
    if verbose:
        print(f"HIBAG model for {obj.hla_locus}: {len(obj.classifiers)} individual classifiers, "
              f"{obj.n_snp} SNPs, {obj.n_hla} unique HLA alleles")

    geno, samp_num = training_cohort(obj, hla, snp, every_classifier=True)
    truth = truth_indices(obj, hla)

    dev = model if isinstance(model, HlaAttrBagClass) else hlaModelFromObj(obj)
    try:
        out = dev.predict_oob_knock(geno, samp_num, truth, call_threshold=call_threshold)
    finally:
        if dev is not model:
            dev.close()
    res = summarise(obj, out["tally"], call_threshold, detail)
    if verbose:
        used = int(np.count_nonzero(res.n_classifier))
        print(f"{out['n_variant']} (classifier, SNP) knock-outs, {used} of {obj.n_snp} SNPs in use")
    return res


__all__ = ["hlaSNPImportance", "HlaSNPImportance"]
