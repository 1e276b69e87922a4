"""``hlaPredictDraws``: a handful of allele pairs per sample drawn from the sample's posterior distribution, on the device.

An analysis that has to carry the imputation's uncertainty -- multiple imputation for an association test, a non-additive,
haplotype or amino-acid model where the allele dosage is not enough -- needs, per sample, allele pairs drawn with the
probabilities ``hlaPredict(type="response+prob")`` reports.  That call sends the whole posterior matrix back (8 * n_cell
bytes per sample) to be sampled on the host; the draw finish (``hibag_hip_predict_draw`` and its routes) reads the ensemble
sums once more on the device and returns n * 20 + 8 bytes per sample.

The draws are defined exactly: the running sum of the posterior in pair order, one uniform per
(seed, sample index, draw) from the counter-based generator Philox4x32-10, the first pair whose running sum exceeds
u * total.  A sample's draws therefore do not depend on how the cohort was batched, on the route the genotypes took or on
how many draws were asked for.  R's ``sample(prob=)`` stream is deliberately not mirrored."""

from __future__ import annotations

from typing import Iterator, List, Optional, Sequence

import numpy as np

from .hibag import HlaAlleleClass, HlaAttrBagClass, draw_n
from .model import NA_INTEGER
from .topk import _predict_lists

_VOTES = ("prob", "majority")


class HlaPosteriorDraws:
    """``n`` allele pairs per sample drawn from its posterior: ``h1`` / ``h2`` [n_samp, n] (0-based indices into
    ``levels``, h1 <= h2, ``NA_INTEGER`` in every draw of a sample without a prediction), ``prob`` [n_samp, n] (the drawn
    pair's posterior probability; 0 or NaN there), ``matching`` [n_samp]; ``seed`` (the seed the draws were made with),
    ``locus``, ``sample_id``, ``n``, ``assembly``, ``levels`` (the model's allele names).  ``draw(t)`` is draw t of every
    sample as an :class:`HlaAlleleClass`; iterating runs over the draws.  ``allele1`` / ``allele2``: per draw the list of
    names (``None`` = NA), made when first read."""

    def __init__(self, locus: str, sample_id: List, n: int, h1: np.ndarray, h2: np.ndarray, prob: np.ndarray,
                 matching: np.ndarray, seed: int = 0, assembly: str = "unknown", levels: Optional[Sequence[str]] = None):
        h1, h2, prob = np.asarray(h1, np.int32), np.asarray(h2, np.int32), np.asarray(prob, np.float64)
        ns = len(sample_id)
        for a in (h1, h2, prob):
            if a.shape != (ns, n):
                raise ValueError(f"expected arrays of shape ({ns}, {n}), got {a.shape}")
        self.locus, self.sample_id, self.n, self.seed = locus, sample_id, int(n), int(seed)
        self.h1, self.h2, self.prob, self.matching = h1, h2, prob, matching
        self.assembly, self.levels = assembly, ([] if levels is None else levels)
        self._allele1 = self._allele2 = None

    def _names_of(self, h: np.ndarray) -> List[List[Optional[str]]]:
        nl = len(self.levels)
        lv = np.empty(nl + 1, dtype=np.object_)
        lv[:nl] = list(self.levels)
        lv[nl] = None
        return [lv.take(np.where(h[:, t] == NA_INTEGER, nl, h[:, t])).tolist() for t in range(self.n)]

    @property
    def allele1(self) -> List[List[Optional[str]]]:
        """``allele1[t][s]``: the first allele's name of sample s's draw t."""
        if self._allele1 is None:
            self._allele1 = self._names_of(self.h1)
        return self._allele1

    @property
    def allele2(self) -> List[List[Optional[str]]]:
        if self._allele2 is None:
            self._allele2 = self._names_of(self.h2)
        return self._allele2

    def draw(self, t: int) -> HlaAlleleClass:
        """Draw ``t`` of every sample as an :class:`HlaAlleleClass` (``hlaCompareAllele(true, draws.draw(0))`` works)."""
        if not isinstance(t, (int, np.integer)) or isinstance(t, bool) or not (0 <= int(t) < self.n):
            raise IndexError(f"draw must be an integer between 0 and {self.n - 1}: {t!r}")
        t = int(t)
        return HlaAlleleClass(locus=self.locus, sample_id=list(self.sample_id), h1=np.ascontiguousarray(self.h1[:, t]),
                              h2=np.ascontiguousarray(self.h2[:, t]), levels=self.levels,
                              prob=np.ascontiguousarray(self.prob[:, t]), matching=self.matching, assembly=self.assembly)

    def __len__(self) -> int:
        return self.n

    def __iter__(self) -> Iterator[HlaAlleleClass]:
        return (self.draw(t) for t in range(self.n))

    def __repr__(self):
        return (f"HlaPosteriorDraws(locus={self.locus!r}, {len(self.sample_id)} samples, n={self.n}, seed={self.seed}, "
                f"assembly={self.assembly!r})")


def hlaPredictDraws(model: HlaAttrBagClass, snp, n: int = 10, seed: Optional[int] = None, vote: str = "prob",
                    allele_check: bool = True, match_type: str = "Position", same_strand: bool = False,
                    verbose: bool = True, verbose_match: bool = True) -> HlaPosteriorDraws:
    """Per sample ``n`` allele pairs drawn from ``hlaPredict(model, snp, vote=vote)``'s posterior matrix, on the device
    (1 <= n <= ``HIBAG_HIP_DRAW_MAX``).

    ``snp``: what ``hlaPredictTopK`` takes -- an :class:`HlaSNPGeno`, a numeric matrix [n.snp, n.samp] in either memory
    order, a vector of length n.snp, a lazily opened :class:`HlaBEDGeno`, or a resident :class:`HlaDeviceCohort`; SNP
    matching, strand flips and missing model SNPs as ``hlaPredict`` decides them.  ``seed``: any integer; ``None`` draws one
    from the module's stream (:func:`set_seed`), as ``hlaConcurrentAttrBagging`` does, so that repeated calls differ and
    ``set_seed(s)`` before the call makes it reproducible; the result reports it.  Draw t of sample s depends on (seed, s, t)
    and the sample's posterior alone: the first draws of a call with a larger ``n`` are the draws of a call with a smaller
    one.  A pair of probability 0 is never drawn; a sample without a positive pair has ``NA_INTEGER`` in every draw."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    n = draw_n(n)
    if seed is None:
        from .train import _R
        seed = int(_R.unif_rand() * 2147483647.0)
    elif not isinstance(seed, (int, np.integer)) or isinstance(seed, (bool, np.bool_)):
        raise ValueError(f"'seed' must be an integer or None: {seed!r}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    vote_method = _VOTES.index(vote) + 1
    what = (str(n) + " posterior draw" + ("s" if n > 1 else "") + " per sample (seed " + str(seed) + "), " +
            ("from the averaged posterior probabilities" if vote_method == 1
             else "from the votes of all individual classifiers"))
    rv, sample_id, assembly = _predict_lists(model, snp, "draw", (n, seed), what, vote_method, allele_check, match_type,
                                             same_strand, verbose, verbose_match)
    return HlaPosteriorDraws(locus=model.obj.hla_locus, sample_id=sample_id, n=n, h1=rv["h1"], h2=rv["h2"], prob=rv["prob"],
                             matching=rv["matching"], seed=seed, assembly=assembly, levels=model.obj.hla_allele)
