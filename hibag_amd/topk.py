"""``hlaPredictTopK``: each sample's k best allele pairs -- "the best guess, the runner-up, and how far apart they are" --
selected on the device.

``hlaPredict`` reports one pair (``type="response"``) or the whole posterior matrix (``type="response+prob"``: 8 * n_cell
bytes per sample, downloaded and sorted on the host).  The top-k finish (``hibag_hip_predict_topk`` and its routes) reads the
ensemble sums once more on the device and returns k * 20 + 8 bytes per sample: the k largest cells of the normalised
posterior matrix, descending, equal values in pair order, cells that are 0 or NaN never listed.  Rank 0 is ``hlaPredict``'s
call bit for bit."""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .hibag import HlaAlleleClass, HlaAttrBagClass, _predict_resolved, _resolve_snp, _warn_no_prediction, topk_k
from .model import NA_INTEGER

_VOTES = ("prob", "majority")


class HlaTopCalls:
    """The k best allele pairs of every sample: ``h1`` / ``h2`` [n_samp, k] (0-based indices into ``levels``, h1 <= h2,
    ``NA_INTEGER`` in the ranks no pair qualifies for), ``prob`` [n_samp, k] (0 there), ``matching`` [n_samp]; ``locus``,
    ``sample_id``, ``k``, ``assembly``, ``levels`` (the model's allele names).  ``allele1`` / ``allele2``: per rank the list
    of names (``None`` = NA), made when first read."""

    def __init__(self, locus: str, sample_id: List, k: int, h1: np.ndarray, h2: np.ndarray, prob: np.ndarray,
                 matching: np.ndarray, assembly: str = "unknown", levels: Optional[Sequence[str]] = None):
        h1, h2, prob = np.asarray(h1, np.int32), np.asarray(h2, np.int32), np.asarray(prob, np.float64)
        n = len(sample_id)
        for a in (h1, h2, prob):
            if a.shape != (n, k):
                raise ValueError(f"expected arrays of shape ({n}, {k}), got {a.shape}")
        self.locus, self.sample_id, self.k = locus, sample_id, int(k)
        self.h1, self.h2, self.prob, self.matching = h1, h2, prob, matching
        self.assembly, self.levels = assembly, ([] if levels is None else levels)
        self._allele1 = self._allele2 = None

    def _names_of(self, h: np.ndarray) -> List[List[Optional[str]]]:
        n = len(self.levels)
        lv = np.empty(n + 1, dtype=np.object_)
        lv[:n] = list(self.levels)
        lv[n] = None
        return [lv.take(np.where(h[:, r] == NA_INTEGER, n, h[:, r])).tolist() for r in range(self.k)]

    @property
    def allele1(self) -> List[List[Optional[str]]]:
        """``allele1[r][s]``: the first allele's name of sample s's rank r."""
        if self._allele1 is None:
            self._allele1 = self._names_of(self.h1)
        return self._allele1

    @property
    def allele2(self) -> List[List[Optional[str]]]:
        if self._allele2 is None:
            self._allele2 = self._names_of(self.h2)
        return self._allele2

    @property
    def n_listed(self) -> np.ndarray:
        """Ranks filled per sample."""
        return np.count_nonzero(self.h1 != NA_INTEGER, axis=1)

    @property
    def coverage(self) -> np.ndarray:
        """The posterior mass the list holds: ``prob.sum(axis=1)``."""
        return self.prob.sum(axis=1)

    def rank(self, r: int) -> HlaAlleleClass:
        """Rank ``r`` of every sample as an :class:`HlaAlleleClass` (``hlaCompareAllele(true, top.rank(1))`` works)."""
        if not isinstance(r, (int, np.integer)) or isinstance(r, bool) or not (0 <= int(r) < self.k):
            raise IndexError(f"rank must be an integer between 0 and {self.k - 1}: {r!r}")
        r = int(r)
        return HlaAlleleClass(locus=self.locus, sample_id=list(self.sample_id), h1=np.ascontiguousarray(self.h1[:, r]),
                              h2=np.ascontiguousarray(self.h2[:, r]), levels=self.levels,
                              prob=np.ascontiguousarray(self.prob[:, r]), matching=self.matching, assembly=self.assembly)

    def best(self) -> HlaAlleleClass:
        """What ``hlaPredict(..., type="response")`` returns: rank 0."""
        return self.rank(0)

    def __repr__(self):
        return f"HlaTopCalls(locus={self.locus!r}, {len(self.sample_id)} samples, k={self.k}, assembly={self.assembly!r})"


def _predict_lists(model: HlaAttrBagClass, snp, family: str, args: tuple, what: str, vote_method: int, allele_check: bool,
                   match_type: str, same_strand: bool, verbose: bool, verbose_match: bool):
    """What ``hlaPredictTopK`` and ``hlaPredictDraws`` share: ``hlaPredict``'s resolution of ``snp`` to a route (with its verbose
    header; ``what``: the line that says what is reported per sample), the call of that route's ``predict_<family>*`` entry,
    and the "No prediction output" warning.  Returns ``(outputs, sample ids, assembly)``."""
    r = _resolve_snp(model.obj, snp, what, match_type, allele_check, same_strand, verbose, verbose_match)
    rv = _predict_resolved(model, snp, r, family, args, vote_method)
    _warn_no_prediction(int(np.count_nonzero((rv["h1"][:, 0] == NA_INTEGER) | (rv["h2"][:, 0] == NA_INTEGER))))
    return rv, list(r.sample_id), r.assembly


def hlaPredictTopK(model: HlaAttrBagClass, snp, k: int = 3, vote: str = "prob", allele_check: bool = True,
                   match_type: str = "Position", same_strand: bool = False, verbose: bool = True,
                   verbose_match: bool = True) -> HlaTopCalls:
    """Per sample the ``k`` most probable allele pairs of ``hlaPredict(model, snp, vote=vote)``'s posterior matrix with
    their probabilities, selected on the device (1 <= k <= ``HIBAG_HIP_TOPK_MAX``).

    ``snp``: what ``hlaPredict`` takes on one device -- an :class:`HlaSNPGeno` (SNP matching, strand flips and missing
    model SNPs as ``hlaPredict`` decides them, applied on the device), a numeric matrix [n.snp, n.samp] in either memory
    order, a vector of length n.snp, a lazily opened :class:`HlaBEDGeno`, or a resident :class:`HlaDeviceCohort`.  The list is descending; equal probabilities
    come in pair order; a pair with probability 0 (or NaN) is never listed, so a sample may have fewer than ``k`` ranks
    filled (``NA_INTEGER`` / 0.0 in the others).  ``best()`` is ``hlaPredict(..., type="response")`` bit for bit."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    k = topk_k(k)
    vote_method = _VOTES.index(vote) + 1
    what = ("the " + str(k) + " best allele pair" + ("s" if k > 1 else "") + " per sample, " +
            ("based on the averaged posterior probabilities" if vote_method == 1
             else "by voting from all individual classifiers"))
    rv, sample_id, assembly = _predict_lists(model, snp, "topk", (k,), what, vote_method, allele_check, match_type,
                                             same_strand, verbose, verbose_match)
    return HlaTopCalls(locus=model.obj.hla_locus, sample_id=sample_id, k=k, h1=rv["h1"], h2=rv["h2"], prob=rv["prob"],
                       matching=rv["matching"], assembly=assembly, levels=model.obj.hla_allele)
