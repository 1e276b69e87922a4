"""``hlaPredictGiven``: allele calls conditioned on what is already known of a sample's type, on the device.

Many cohorts carry partial typing at the locus: serology, two-digit types, one allele typed and the other not, an ambiguity
list of sequence-based typing ("01:01/01:02").  What the user wants is the four-digit call CONSISTENT with it.  The
constraint is a per-sample input: two allele sets A and B over the model's alleles, and a pair (h1, h2) is consistent when
one allele lies in A and the other in B.  ``hlaPredict(type="response+prob")`` returns the matrix to mask on the host,
8 * n_cell bytes per sample; the given finish (``hibag_hip_predict_given`` and its routes) reads the ensemble sums once on
the device and returns 24 bytes per sample, plus 8 per allele with the dosages.  The result is defined exactly (DESIGN.md
section 18): with both sets full it is ``hlaPredict``'s call, probability and dosage bit for bit.

No serology or sequence database is shipped: the builders take the names the caller brings."""

from __future__ import annotations

import sys
from typing import Iterable, List, Optional, Sequence, Union

import numpy as np

from .bed import HlaBEDGeno
from .cohort import HlaDeviceCohort
from .hibag import HlaAlleleClass, HlaAttrBagClass, _predict_resolved, _resolve_snp, _warn_no_prediction
from .model import NA_INTEGER, HlaSNPGeno

_VOTES = ("prob", "majority")


def _alleles_of(model_or_alleles) -> List[str]:
    obj = getattr(model_or_alleles, "obj", model_or_alleles)
    return [str(a) for a in getattr(obj, "hla_allele", obj)]


def _words(n_hla: int) -> int:
    return (int(n_hla) + 31) // 32


class HlaAlleleConstraint:
    """Per sample two sets of a model's alleles: ``alleles`` (the model's ``hla_allele``), ``allowed`` bool
    [n_samp, 2, n_hla] (``allowed[s, 0]`` is set A, ``allowed[s, 1]`` set B), ``sample_id`` (a list, or ``None`` if not
    known: the rows are then the genotypes' samples in order) and ``n_unmatched`` (names given to a builder that match no
    allele of the model)."""

    def __init__(self, alleles: Sequence[str], allowed, sample_id: Optional[Sequence] = None, n_unmatched: int = 0):
        self.alleles = [str(a) for a in alleles]
        a = np.asarray(allowed)
        if a.dtype != np.bool_ or a.ndim != 3 or a.shape[1:] != (2, len(self.alleles)):
            raise ValueError(f"allowed must be a boolean array [n_samp, 2, n_hla = {len(self.alleles)}], got {a.dtype} {a.shape}")
        if len(self.alleles) < 1:
            raise ValueError("no allele given")
        self.allowed = np.ascontiguousarray(a)
        self.sample_id = None if sample_id is None else list(sample_id)
        if self.sample_id is not None and len(self.sample_id) != a.shape[0]:
            raise ValueError("one sample id per row of allowed")
        self.n_unmatched = int(n_unmatched)

    @classmethod
    def from_packed(cls, alleles: Sequence[str], packed, sample_id: Optional[Sequence] = None) -> "HlaAlleleConstraint":
        """From the uint32 form [n_samp, 2, W] (:meth:`pack`); bits at or above n_hla are dropped."""
        n = len(alleles)
        p = np.asarray(packed)
        if p.dtype != np.uint32 or p.ndim != 3 or p.shape[1:] != (2, _words(n)):
            raise ValueError(f"expected a uint32 array [n_samp, 2, W = {_words(n)}], got {p.dtype} {p.shape}")
        bits = np.unpackbits(np.ascontiguousarray(p.astype("<u4")).view(np.uint8), axis=2, bitorder="little")
        return cls(alleles, bits[:, :, :n].astype(np.bool_), sample_id)

    @property
    def n_samp(self) -> int:
        return int(self.allowed.shape[0])

    @property
    def n_hla(self) -> int:
        return len(self.alleles)

    def pack(self) -> np.ndarray:
        """uint32 [n_samp, 2, W], W = (n_hla + 31) // 32: allele h is bit h % 32 of word h // 32 (the C form ``allow``)."""
        n, w = self.n_hla, _words(self.n_hla)
        padded = np.zeros((self.n_samp, 2, w * 32), np.uint8)
        padded[:, :, :n] = self.allowed
        return np.ascontiguousarray(np.packbits(padded, axis=2, bitorder="little").view("<u4").astype(np.uint32))

    def constrained(self) -> np.ndarray:
        """[n_samp]: on how many of the two chromosomes the sample is constrained (a set that is not all alleles)."""
        return np.count_nonzero(~self.allowed.all(axis=2), axis=1)

    def rows_for(self, sample_id: Sequence) -> "HlaAlleleConstraint":
        """The constraint of the samples ``sample_id``, in that order, matched by id; a sample this object does not hold is
        unconstrained (both sets full)."""
        if self.sample_id is None:
            raise ValueError("the constraint carries no sample ids")
        at = {}
        for i, sid in enumerate(self.sample_id):
            at.setdefault(sid, i)
        idx = np.array([at.get(sid, -1) for sid in sample_id], np.int64)
        out = np.ones((len(idx), 2, self.n_hla), np.bool_)
        have = idx >= 0
        out[have] = self.allowed[idx[have]]
        return HlaAlleleConstraint(self.alleles, out, list(sample_id), self.n_unmatched)

    def __len__(self) -> int:
        return self.n_samp

    def __repr__(self):
        c = self.constrained()
        return (f"HlaAlleleConstraint({self.n_samp} samples over {self.n_hla} alleles: {int(np.count_nonzero(c == 2))} constrained "
                f"on two chromosomes, {int(np.count_nonzero(c == 1))} on one; {self.n_unmatched} unmatched names)")


def _match_name(fields_of: List[List[str]], name: str) -> np.ndarray:
    """The model alleles whose leading ':'-fields equal the fields of ``name`` (``hlaAlleleDigit``'s notion of fields)."""
    k = str(name).strip().split(":")
    return np.array([f[:len(k)] == k for f in fields_of], np.bool_)


def _is_na(x) -> bool:
    return x is None or (isinstance(x, float) and x != x)


def hlaConstraintFromAllele(model_or_alleles, hla, unmatched: str = "empty") -> HlaAlleleConstraint:
    """The constraint a (partially) typed cohort makes.  ``hla``: an :class:`HlaAlleleClass` whose ``allele1`` / ``allele2``
    may be of lower resolution than the model's ("02", "02:01" against "02:01:01"): a name selects every model allele whose
    leading ':'-fields equal it; ``None`` (NA) selects all alleles.  A name that matches no allele of the model gives an empty
    set -- nothing is consistent, the call is NA -- or, with ``unmatched="free"``, the full set; either way it is counted in
    ``n_unmatched``.  ``allele1`` makes set A, ``allele2`` set B; ``hla.sample_id`` is kept."""
    if unmatched not in ("empty", "free"):
        raise ValueError("'unmatched' should be one of \"empty\", \"free\"")
    alleles = _alleles_of(model_or_alleles)
    a1, a2 = list(hla.allele1), list(hla.allele2)
    if len(a1) != len(a2):
        raise ValueError("allele1 and allele2 differ in length")
    fields_of = [a.split(":") for a in alleles]
    allowed = np.ones((len(a1), 2, len(alleles)), np.bool_)
    cache, n_un = {}, 0
    for j, names in enumerate((a1, a2)):
        for s, name in enumerate(names):
            if _is_na(name):
                continue
            if name not in cache:
                cache[name] = _match_name(fields_of, name)
            sel = cache[name]
            if not sel.any():
                n_un += 1
                if unmatched == "free":
                    continue
            allowed[s, j] = sel
    return HlaAlleleConstraint(alleles, allowed, getattr(hla, "sample_id", None), n_un)


def _names_of_set(x) -> Optional[List[str]]:
    if _is_na(x):
        return None
    if isinstance(x, str):
        return [t.strip() for t in x.split("/") if t.strip()]
    return [str(t) for t in x]


def hlaConstraintFromSets(model_or_alleles, set1: Sequence, set2: Sequence,
                          sample_id: Optional[Sequence] = None) -> HlaAlleleConstraint:
    """The constraint two lists of allele sets make: per sample and chromosome an iterable of names or one "/"-separated
    string (an ambiguity list, "01:01/01:02"); ``None`` means all alleles.  Every name selects as in
    :func:`hlaConstraintFromAllele`, a set is the union of its names; a name that matches nothing adds nothing and is counted
    in ``n_unmatched``."""
    alleles = _alleles_of(model_or_alleles)
    set1, set2 = list(set1), list(set2)
    if len(set1) != len(set2):
        raise ValueError("set1 and set2 differ in length")
    fields_of = [a.split(":") for a in alleles]
    allowed = np.ones((len(set1), 2, len(alleles)), np.bool_)
    cache, n_un = {}, 0
    for j, sets in enumerate((set1, set2)):
        for s, x in enumerate(sets):
            names = _names_of_set(x)
            if names is None:
                continue
            sel = np.zeros(len(alleles), np.bool_)
            for name in names:
                if name not in cache:
                    cache[name] = _match_name(fields_of, name)
                if not cache[name].any():
                    n_un += 1
                sel |= cache[name]
            allowed[s, j] = sel
    return HlaAlleleConstraint(alleles, allowed, sample_id, n_un)


class HlaGivenCalls:
    """Per sample the best allele pair consistent with its constraint: ``h1`` / ``h2`` [n_samp] (0-based indices into
    ``alleles``, h1 <= h2, ``NA_INTEGER`` where no consistent pair qualifies), ``prob`` (CONDITIONAL on the constraint:
    ``prob_joint / support`` where ``support > 0``, the joint value as it is elsewhere), ``prob_joint`` (the pair's
    posterior), ``support`` (the posterior mass of the consistent pairs), ``matching``, ``dosage`` [n_hla, n_samp] or ``None``
    (conditional in the same way); ``constraint``, ``locus``, ``sample_id``, ``assembly``."""

    def __init__(self, locus: str, sample_id: List, alleles: Sequence[str], h1: np.ndarray, h2: np.ndarray,
                 prob_joint: np.ndarray, support: np.ndarray, matching: np.ndarray, dosage_joint: Optional[np.ndarray] = None,
                 constraint: Optional[HlaAlleleConstraint] = None, assembly: str = "unknown"):
        self.locus, self.sample_id, self.alleles, self.assembly = locus, sample_id, list(alleles), assembly
        self.h1, self.h2, self.prob_joint, self.support, self.matching = h1, h2, prob_joint, support, matching
        self.constraint = constraint
        pos = support > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            self.prob = np.where(pos, prob_joint / np.where(pos, support, 1.0), prob_joint)
            self.dosage = None
            if dosage_joint is not None:                      # [n_samp, n_hla] from the device -> hlaPredict's [n_hla, n_samp]
                self.dosage = np.where(pos[:, None], dosage_joint / np.where(pos, support, 1.0)[:, None], dosage_joint).T

    def calls(self) -> HlaAlleleClass:
        """The calls as an :class:`HlaAlleleClass` like ``hlaPredict``'s, with the conditional probability and dosage."""
        return HlaAlleleClass(locus=self.locus, sample_id=list(self.sample_id), h1=self.h1, h2=self.h2, levels=self.alleles,
                              prob=self.prob, matching=self.matching, assembly=self.assembly, dosage=self.dosage)

    def __repr__(self):
        return f"HlaGivenCalls(locus={self.locus!r}, {len(self.sample_id)} samples, assembly={self.assembly!r})"


def _constraint_for(model: HlaAttrBagClass, known, snp, sample_id: Sequence, n_samp: int) -> HlaAlleleConstraint:
    alleles = [str(a) for a in model.obj.hla_allele]
    if not isinstance(known, HlaAlleleConstraint):
        a = np.asarray(known)
        if a.dtype == np.bool_:
            known = HlaAlleleConstraint(alleles, a)
        elif a.dtype == np.uint32:
            known = HlaAlleleConstraint.from_packed(alleles, a)
        else:
            raise TypeError("'known' must be an HlaAlleleConstraint, a boolean array [n_samp, 2, n_hla] or a uint32 array "
                            "[n_samp, 2, W]")
    if known.alleles != alleles:
        raise ValueError("'known' constrains another allele list than the model's")
    if known.sample_id is not None and isinstance(snp, (HlaSNPGeno, HlaBEDGeno, HlaDeviceCohort)):
        return known.rows_for(list(sample_id))
    if known.n_samp != n_samp:
        raise ValueError(f"'known' holds {known.n_samp} samples, 'snp' {n_samp} (without sample ids on both sides the rows "
                         "are taken in order)")
    return known


def hlaPredictGiven(model: HlaAttrBagClass, snp, known: Union[HlaAlleleConstraint, np.ndarray], dosage: bool = False,
                    vote: str = "prob", allele_check: bool = True, match_type: str = "Position", same_strand: bool = False,
                    verbose: bool = True, verbose_match: bool = True) -> HlaGivenCalls:
    """Per sample the most probable allele pair under ``hlaPredict(model, snp, vote=vote)``'s posterior AMONG THE PAIRS
    CONSISTENT WITH ``known``, its conditional and joint probability, the posterior mass of the consistent pairs and
    (``dosage``) the conditional allele dosages, on the device.

    ``known``: an :class:`HlaAlleleConstraint` over the model's alleles (:func:`hlaConstraintFromAllele`,
    :func:`hlaConstraintFromSets`), a boolean array [n_samp, 2, n_hla] or its uint32 form [n_samp, 2, W].  When the
    constraint and ``snp`` both carry sample ids the rows are matched by id and samples absent from ``known`` are
    unconstrained; otherwise the rows are the samples of ``snp`` in order.  ``snp``: what ``hlaPredictGroups`` takes -- an
    :class:`HlaSNPGeno` in either memory order, a numeric matrix [n.snp, n.samp] or a vector, a lazily opened
    :class:`HlaBEDGeno`, a resident :class:`HlaDeviceCohort` --, matched as ``hlaPredict`` matches it.  With an
    unconstrained sample the result is ``hlaPredict``'s own call, probability and dosage."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    vote_method = _VOTES.index(vote) + 1
    what = ("the best allele pair consistent with the known partial typing" + (", with conditional dosages" if dosage else "") + ", "
            + ("based on the averaged posterior probabilities" if vote_method == 1 else "by voting from all individual classifiers"))
    r = _resolve_snp(model.obj, snp, what, match_type, allele_check, same_strand, verbose, verbose_match)
    con = _constraint_for(model, known, snp, r.sample_id, r.n_samp)
    if verbose:
        c = con.constrained()
        print(f"Constraint: {int(np.count_nonzero(c == 2))} samples constrained on two chromosomes, {int(np.count_nonzero(c == 1))} "
              f"on one, {int(np.count_nonzero(c == 0))} on none; {con.n_unmatched} unmatched names", file=sys.stdout)
    rv = _predict_resolved(model, snp, r, "given", (con.pack(),), vote_method, want_dosage=bool(dosage))
    _warn_no_prediction(int(np.count_nonzero((rv["h1"] == NA_INTEGER) | (rv["h2"] == NA_INTEGER))))
    return HlaGivenCalls(locus=model.obj.hla_locus, sample_id=list(r.sample_id), alleles=model.obj.hla_allele, h1=rv["h1"],
                         h2=rv["h2"], prob_joint=rv["prob"], support=rv["support"], matching=rv["matching"],
                         dosage_joint=rv.get("dosage"), constraint=con, assembly=r.assembly)
