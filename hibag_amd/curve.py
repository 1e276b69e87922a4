"""``hlaPredictCurve``: the prediction of every ensemble size of one model -- "how many classifiers does this model
need?" -- in one pass over the cohort.

By hand (the reference's way) the curve is a loop: ``hlaSubModelObj(obj, k)`` -> ``hlaModelFromObj`` -> ``hlaPredict``
for every k, K model layouts and K (K + 1) / 2 classifiers' worth of haplotype pairs.  ``hibag_hip_predict_prefix`` does
one pack and one pass 1 over the K classifiers and a read-back fold per size; every call, probability and matching
proportion is bit-identical to the loop's."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Union

import numpy as np

from .bed import HlaBEDGeno
from .evaluate import hlaCompareAllele
from .hibag import HlaAlleleClass, HlaAttrBagClass, _as_integer, hlaModelFromObj
from .model import NA_INTEGER, HlaAttrBagObj, HlaSNPGeno


@dataclass
class HlaPredictCurve:
    """``sizes[i]`` classifiers -> ``pred[i]`` (an :class:`HlaAlleleClass` with ``h1`` / ``h2``, ``prob``, ``matching``; no
    dosage, no posterior matrix), ``changed[i]`` = samples whose unordered call differs from the call at the largest size,
    ``accuracy[i]`` = the allele accuracy ``acc.haplo`` of ``overall[i]`` = ``hlaCompareAllele(hla, pred[i])``'s ``overall`` row
    (``None`` / empty without true types)."""
    sizes: np.ndarray
    pred: List[HlaAlleleClass]
    changed: np.ndarray
    accuracy: Optional[np.ndarray] = None
    overall: List = field(default_factory=list)


def curve_sizes(sizes, n_classifier: int) -> np.ndarray:
    """The ``sizes`` argument as int32, strictly ascending within 1 .. n_classifier; ``None`` = every size."""
    if n_classifier < 1:
        raise ValueError("the model has no classifiers")
    if sizes is None:
        return np.arange(1, n_classifier + 1, dtype=np.int32)
    a = np.asarray(sizes)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("'sizes' must be a non-empty vector")
    if a.dtype.kind not in "iuf" or (a.dtype.kind == "f" and not np.all(a == np.floor(a))):
        raise ValueError("'sizes' must hold whole numbers")
    a = a.astype(np.int64)
    if a.min() < 1 or a.max() > n_classifier:
        raise ValueError(f"'sizes' must lie between 1 and the number of classifiers ({n_classifier})")
    if np.any(np.diff(a) <= 0):
        raise ValueError("'sizes' must be strictly ascending")
    return a.astype(np.int32)


def curve_from_arrays(obj: HlaAttrBagObj, sizes: np.ndarray, sample_id: Sequence, h1: np.ndarray, h2: np.ndarray,
                      prob: np.ndarray, matching: np.ndarray, assembly: str = "unknown",
                      hla: Optional[HlaAlleleClass] = None) -> HlaPredictCurve:
    """The result object from the entry's raw arrays (each [n_sizes, n_samp]; calls are 0-based allele indices with
    h1 <= h2, NA = INT_MIN) -- no per-sample Python objects unless accuracies are asked for."""
    sizes = np.asarray(sizes, np.int32)
    h1, h2 = np.asarray(h1, np.int32), np.asarray(h2, np.int32)
    n = len(sample_id)
    for a in (h1, h2, prob, matching):
        if np.shape(a) != (len(sizes), n):
            raise ValueError(f"expected arrays of shape ({len(sizes)}, {n}), got {np.shape(a)}")
    pred = [HlaAlleleClass(locus=obj.hla_locus, sample_id=list(sample_id), h1=h1[i], h2=h2[i], levels=obj.hla_allele,
                           prob=np.asarray(prob)[i], matching=np.asarray(matching)[i], assembly=assembly)
            for i in range(len(sizes))]
    lo, hi = np.minimum(h1, h2), np.maximum(h1, h2)           # unordered pairs (NA = INT_MIN sorts first in both)
    changed = np.count_nonzero((lo != lo[-1]) | (hi != hi[-1]), axis=1).astype(np.int64)
    accuracy, overall = None, []
    if hla is not None:
        overall = [hlaCompareAllele(hla, p) for p in pred]
        accuracy = np.array([o["acc.haplo"] for o in overall], np.float64)
    return HlaPredictCurve(sizes=sizes, pred=pred, changed=changed, accuracy=accuracy, overall=overall)


def _aligned_matrix(model: HlaAttrBagClass, snp, same_strand: bool, match_type: str, verbose: bool):
    """(int32 [n_samp, model SNPs] in model order, sample ids, assembly): hlaPredict's SNP matching and strand handling
    (``plan_snps_for_predict``), applied on the host to the model's few hundred rows of the cohort."""
    obj = model.obj
    if isinstance(snp, HlaBEDGeno):
        raise TypeError("hlaPredictCurve takes an hlaSNPGenoClass or a genotype matrix; load the BED file first (hlaBED2Geno())")
    if not isinstance(snp, HlaSNPGeno):
        g = np.asarray(snp)
        if g.dtype.kind not in "iufb":
            raise TypeError("is.numeric(snp) is not TRUE")
        if g.ndim == 1:
            if g.shape[0] != obj.n_snp:
                raise ValueError("length(snp) == object$n.snp is not TRUE")
            g = g.reshape(-1, 1)
        elif g.ndim != 2 or g.shape[0] != obj.n_snp:
            raise ValueError("nrow(snp) == object$n.snp is not TRUE")
        return np.ascontiguousarray(_as_integer(g).T, np.int32), list(range(1, g.shape[1] + 1)), "auto-silent"
    from .snpmatch import _row_afreq, plan_snps_for_predict
    mat = np.asarray(snp.genotype)
    if mat.ndim != 2:
        raise ValueError("'snp$genotype' must be a matrix [n.snp, n.samp]")
    if len(snp.sample_id) != mat.shape[1]:
        raise ValueError("length(snp$sample.id) == ncol(snp$genotype) is not TRUE")
    plan = plan_snps_for_predict(obj, snp, lambda rows: _row_afreq(_as_integer(mat[rows])), match_type, True, same_strand,
                                 verbose, verbose)
    g = _as_integer(mat)
    idx = np.arange(obj.n_snp) if plan.identity else np.asarray(plan.sel)
    rows = np.array(g[np.maximum(idx, 0)], np.int32)
    if plan.flip is not None and np.any(plan.flip):
        fl = np.asarray(plan.flip, bool)[:, None]
        rows = np.where(fl & (rows >= 0) & (rows <= 2), 2 - rows, rows)
    rows[idx < 0] = NA_INTEGER
    return np.ascontiguousarray(rows.T, np.int32), list(snp.sample_id), plan.assembly


def hlaPredictCurve(model: Union[HlaAttrBagClass, HlaAttrBagObj], snp, sizes=None, hla: Optional[HlaAlleleClass] = None,
                    same_strand: bool = False, match_type: str = "Position", verbose: bool = True) -> HlaPredictCurve:
    """For every ensemble size in ``sizes`` (default 1 .. n_classifier) the prediction -- vote by averaged posterior
    probabilities -- of the model made of the first that many classifiers (``hlaSubModelObj``), each bit-identical to
    ``hlaPredict(hlaModelFromObj(hlaSubModelObj(obj, k)), snp, type="response")``.

    ``model``: an :class:`HlaAttrBagClass`, or an :class:`HlaAttrBagObj` (a temporary device model, closed afterwards).
    ``snp``: what ``hlaPredict`` takes (an :class:`HlaSNPGeno` or a numeric matrix [n.snp, n.samp]); SNP matching and
    strand handling are ``hlaPredict``'s.  ``hla``: the true types; with them ``accuracy`` is filled in."""
    own = isinstance(model, HlaAttrBagObj)
    if not own and not isinstance(model, HlaAttrBagClass):
        raise TypeError("'model' must be an hlaAttrBagClass or an hlaAttrBagObj")
    if hla is not None and not isinstance(hla, HlaAlleleClass):
        raise TypeError("inherits(hla, \"hlaAlleleClass\") is not TRUE")
    obj = model if own else model.obj
    sz = curve_sizes(sizes, len(obj.classifiers))
    dev = hlaModelFromObj(model) if own else model
    try:
        genomat, sample_id, assembly = _aligned_matrix(dev, snp, same_strand, match_type, verbose)
        if verbose:
            print(f"HIBAG model for HLA-{obj.hla_locus}: {len(obj.classifiers)} individual classifiers, "
                  f"{len(sz)} ensemble sizes from {int(sz[0])} to {int(sz[-1])}\n# of samples: {genomat.shape[0]}")
        rv = dev.predict_prefix(genomat, sz)
    finally:
        if own:
            dev.close()
    return curve_from_arrays(obj, sz, sample_id, rv["h1"], rv["h2"], rv["prob"], rv["matching"], assembly, hla)
