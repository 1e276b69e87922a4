"""``hlaDistance`` (``R/HIBAG.R:1545-1570``): the frequency-weighted mean number of differing SNPs between the haplotypes
of every pair of alleles, per classifier (``HIBAG_Distance``, ``src/HIBAG.cpp:1284-1332``) and averaged over the
classifiers that have haplotypes of both alleles.  Users cluster it (``hclust(as.dist(d))``) to see which alleles a
model tells apart.

The reference calls its C routine once per classifier and folds the matrices in R.  Here one device call
(``hibag_hip_model_distance``) does both, bit-identical to the reference (DESIGN.md "hlaDistance").

Deviation: a model without classifiers raises ``ValueError`` (R would return an empty result)."""

from __future__ import annotations

import ctypes as C
from typing import Tuple, Union

import numpy as np

from . import _lib
from ._lib import HibagHipError
from .hibag import HlaAttrBagClass, _as_ptr
from .model import HlaAttrBagObj


def _unfinalized_handle(obj: HlaAttrBagObj) -> C.c_void_p:
    """A native model with ``obj``'s classifiers that is never finalized: the distance needs no prediction layout.
    The classifier checks are hlaModelFromObj's (haplotypes grouped by ascending allele, '0'/'1' strings, ...)."""
    L = _lib.lib()
    h = L.hibag_hip_model_new(int(obj.n_hla), int(obj.n_snp))
    if not h:
        raise HibagHipError(-1, L.hibag_hip_last_error().decode())
    h = C.c_void_p(h)
    try:
        for c in obj.classifiers:
            strs = (C.c_char_p * len(c.haplo))(*[s.encode() for s in c.haplo])
            _lib.check(L.hibag_hip_model_add_classifier(
                h, len(c.snpidx), _as_ptr(c.snpidx), len(c.freq), _as_ptr(c.freq), _as_ptr(c.hla), strs))
    except Exception:
        L.hibag_hip_model_free(h)
        raise
    return h


def hlaDistance(model: Union[HlaAttrBagObj, HlaAttrBagClass], classifiers: bool = False
                ) -> Union[np.ndarray, Tuple[np.ndarray, np.ndarray]]:
    """The ``[n_hla, n_hla]`` float64 distance matrix of ``model``, rows and columns in ``hla_allele`` order (R's dimnames).
    NaN where no classifier has a haplotype pair of the two alleles.

    ``classifiers=True`` also returns each classifier's matrix, ``[n_classifier, n_hla, n_hla]`` with NaN kept (R's
    ``lst`` before ``m[is.na(m)] <- 0``).  An ``HlaAttrBagClass`` is computed from its resident handle; an
    ``HlaAttrBagObj`` through a temporary native model that is freed afterwards."""
    if not isinstance(model, (HlaAttrBagObj, HlaAttrBagClass)):
        raise TypeError('inherits(model, "hlaAttrBagObj") | inherits(model, "hlaAttrBagClass") is not TRUE')
    if not isinstance(classifiers, (bool, np.bool_)):
        raise TypeError("'classifiers' should be TRUE or FALSE.")
    obj = model.obj if isinstance(model, HlaAttrBagClass) else model
    nclass, n = len(obj.classifiers), int(obj.n_hla)
    if nclass == 0:
        raise ValueError("hlaDistance: the model has no classifier.")
    L = _lib.lib()
    out = np.empty((n, n), np.float64)
    each = np.empty((nclass, n, n), np.float64) if classifiers else None
    if isinstance(model, HlaAttrBagClass):
        _lib.check(L.hibag_hip_model_distance(model.handle, _as_ptr(out), _as_ptr(each)))
    else:
        h = _unfinalized_handle(obj)
        try:
            _lib.check(L.hibag_hip_model_distance(h, _as_ptr(out), _as_ptr(each)))
        finally:
            L.hibag_hip_model_free(h)
    return (out, each) if classifiers else out
