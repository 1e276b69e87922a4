"""``hlaSubModelObj`` and ``hlaCombineModelObj`` (``R/HIBAG.R:1121-1129``, ``:1069-1114``): a model of the first n
classifiers of another, and two models of one locus put together.  Host-side list surgery on :class:`HlaAttrBagObj`;
nothing here touches the device."""

from __future__ import annotations

import dataclasses
from typing import Any, List, Optional

import numpy as np

from . import rdata
from .model import HlaAttrBagObj


def hlaSubModelObj(obj: HlaAttrBagObj, n: int) -> HlaAttrBagObj:
    """``hlaSubModelObj(obj, n)``: ``obj`` with ``classifiers[1:n]``, every other field unchanged (and shared, not
    copied: R's copy-on-modify gives the same).

    Deviation from the reference: ``n < 1`` or ``n > length(obj$classifiers)`` raises ``ValueError``.  R's ``1L:n`` counts
    DOWN for ``n < 1`` (``1:0`` is ``c(1, 0)``: the first classifier) and pads with NULL entries beyond the end -- models
    that ``hlaModelFromObj`` then rejects or misreads -- so there is nothing useful to reproduce."""
    if not isinstance(obj, HlaAttrBagObj):
        raise TypeError("inherits(obj, \"hlaAttrBagObj\") is not TRUE")
    if isinstance(n, bool) or not isinstance(n, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(n) is not TRUE")
    if n != int(n):
        raise ValueError("n must be a whole number")
    n = int(n)
    if n < 1 or n > len(obj.classifiers):
        raise ValueError(f"n must be between 1 and the number of classifiers ({len(obj.classifiers)}): {n}")
    return dataclasses.replace(obj, classifiers=list(obj.classifiers[:n]))


def _identical(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return list(a) == list(b)


def _appendix_field(appendix: Any, key: str) -> List:
    if appendix is None:
        return []
    v = appendix.get(key) if hasattr(appendix, "get") else None
    if v is None:
        return []
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]


def _unique(items: List) -> List:
    out: List = []
    for x in items:
        if x not in out:
            out.append(x)
    return out


def hlaCombineModelObj(obj1: HlaAttrBagObj, obj2: HlaAttrBagObj) -> HlaAttrBagObj:
    """``hlaCombineModelObj(obj1, obj2)``: one model with the classifiers of both, ``obj1``'s first.

    Like the reference it stops unless locus, ``snp.id``, ``hla.allele`` and assembly are identical.  ``sample.id`` is the
    union in order of first appearance, ``snp.allele.freq`` and ``hla.freq`` are ``(a + b) * 0.5``; ``matching`` is the
    two vectors concatenated, or -- when the two ``sample.id`` vectors are identical and not NULL --
    ``n1/n*m1 + n2/n*m2`` with n1, n2 the numbers of classifiers, in that operation order; the ``appendix`` fields
    ``platform``, ``information`` and ``warning`` are merged by ``unique`` (NULL when neither model has an appendix)."""
    for o in (obj1, obj2):
        if not isinstance(o, HlaAttrBagObj):
            raise TypeError("inherits(obj, \"hlaAttrBagObj\") is not TRUE")
    if obj1.hla_locus != obj2.hla_locus:
        raise ValueError("identical(obj1$hla.locus, obj2$hla.locus) is not TRUE")
    if not _identical(obj1.snp_id, obj2.snp_id):
        raise ValueError("identical(obj1$snp.id, obj2$snp.id) is not TRUE")
    if not _identical(obj1.hla_allele, obj2.hla_allele):
        raise ValueError("identical(obj1$hla.allele, obj2$hla.allele) is not TRUE")
    if obj1.assembly != obj2.assembly:
        raise ValueError("identical(obj1$assembly, obj2$assembly) is not TRUE")

    samp_id = _unique(list(obj1.sample_id) + list(obj2.sample_id))
    appendix: Optional[Any] = None
    if obj1.appendix is not None or obj2.appendix is not None:
        keys = ["platform", "information", "warning"]
        vals = [_unique(_appendix_field(obj1.appendix, k) + _appendix_field(obj2.appendix, k)) for k in keys]
        appendix = rdata.RList([rdata.RStrings(v) if v else None for v in vals], {"names": keys})

    def mean(a, b):
        if a is None or b is None:
            return None                      # (NULL + x is numeric(0) in R: nothing to keep)
        return (np.asarray(a, np.float64) + np.asarray(b, np.float64)) * 0.5

    m1, m2 = obj1.matching, obj2.matching
    parts = [np.asarray(m, np.float64) for m in (m1, m2) if m is not None]
    matching = np.concatenate(parts) if parts else None
    if _identical(obj1.sample_id, obj2.sample_id) and obj1.sample_id is not None and len(obj1.sample_id) > 0 \
            and m1 is not None and m2 is not None:
        n1, n2 = len(obj1.classifiers), len(obj2.classifiers)
        n = n1 + n2
        matching = n1 / n * np.asarray(m1, np.float64) + n2 / n * np.asarray(m2, np.float64)

    return HlaAttrBagObj(
        n_samp=len(samp_id), n_snp=obj1.n_snp, hla_allele=list(obj1.hla_allele),
        classifiers=list(obj1.classifiers) + list(obj2.classifiers), hla_locus=obj1.hla_locus, sample_id=samp_id,
        snp_id=list(obj1.snp_id), snp_position=obj1.snp_position, snp_allele=list(obj1.snp_allele),
        snp_allele_freq=mean(obj1.snp_allele_freq, obj2.snp_allele_freq), hla_freq=mean(obj1.hla_freq, obj2.hla_freq),
        assembly=obj1.assembly, matching=matching, appendix=appendix)
