"""``hlaPredictGroups``: calls under the posterior collapsed over GROUPS of alleles, on the device.

Imputed HLA types are mostly analysed at a coarser level than the four-digit allele pair: two-digit types, P / G groups,
serological groups (Bw4 / Bw6, the C1 / C2 KIR ligands, supertypes), the amino acid at a position of the protein.  Each of
these partitions the model's alleles into groups, and the right call at that level is the maximum of the COLLAPSED posterior:
the pair posterior summed over all allele pairs that fall into each pair of groups.  Relabelling the allele-level best guess
(``hlaAlleleDigit`` on ``allele1`` / ``allele2``) gives another call where the posterior is spread over several alleles of
one group, and a much lower probability nearly everywhere -- the probability ``call_threshold`` filters on.

``hlaPredict(type="response+prob")`` returns the matrix to collapse on the host, 8 * n_cell bytes per sample and one
scatter-add per partition (an amino-acid analysis has 50-150 of them).  The group finish (``hibag_hip_predict_groups`` and its
routes) reads the ensemble sums once on the device and returns n_part * 16 + 8 bytes per sample, plus 8 per group with the
expected group dosages.  The result is defined exactly: with the identity partition it is
``hlaPredict``'s call, probability and dosage bit for bit.

No sequence database is shipped: :func:`hlaGroupsBySequence` takes the aligned sequences the caller brings."""

from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Union

import numpy as np

from . import _lib
from .hibag import GroupsPlan, HlaAlleleClass, HlaAttrBagClass, _predict_resolved, _resolve_snp, _warn_no_prediction
from .merge import hlaAlleleDigit
from .model import NA_INTEGER

_VOTES = ("prob", "majority")


class HlaAlleleGroups:
    """Partitions of an allele list into groups: ``alleles`` (the model's ``hla_allele``), ``names`` [n_part] (what each
    partition is called), ``levels[q]`` (the group names of partition q) and ``group_of`` int32 [n_part, n_hla] (the group of
    every allele, an index into ``levels[q]``).  Groups are numbered in the order of their first appearance along
    ``alleles``.  ``a + b`` holds the partitions of ``a``, then those of ``b`` (over the same alleles)."""

    def __init__(self, alleles: Sequence[str], names: Sequence[str], levels: Sequence[Sequence[str]], group_of):
        self.alleles = list(alleles)
        self.names = [str(n) for n in names]
        self.levels = [list(lv) for lv in levels]
        g = np.asarray(group_of)
        if g.dtype.kind not in "iu" or g.ndim != 2 or g.shape != (len(self.names), len(self.alleles)):
            raise ValueError(f"group_of must be an integer matrix [n_part = {len(self.names)}, n_hla = {len(self.alleles)}], "
                             f"got {g.dtype} {g.shape}")
        if len(self.levels) != len(self.names):
            raise ValueError("one list of levels per partition")
        if len(self.names) < 1:
            raise ValueError("no partition given")
        if len(self.alleles) < 1:
            raise ValueError("no allele given")
        if g.min() < 0 or g.max() >= len(self.alleles):
            raise ValueError(f"group ids must lie in 0 .. n_hla - 1 = {len(self.alleles) - 1}")
        for q, lv in enumerate(self.levels):
            if int(g[q].max()) >= len(lv):
                raise ValueError(f"partition {self.names[q]!r} uses group {int(g[q].max())} but names {len(lv)} levels")
        self.group_of = np.ascontiguousarray(g, np.int32)

    @classmethod
    def from_labels(cls, alleles: Sequence[str], name: str, labels: Sequence[str]) -> "HlaAlleleGroups":
        """One partition from a label per allele: equal labels are one group, numbered by first appearance."""
        if len(labels) != len(alleles):
            raise ValueError("one label per allele")
        index: Dict[str, int] = {}
        ids = [index.setdefault(lab, len(index)) for lab in labels]
        return cls(alleles, [name], [list(index)], np.array([ids], np.int32))

    @classmethod
    def from_matrix(cls, alleles: Sequence[str], group_of, names: Optional[Sequence[str]] = None) -> "HlaAlleleGroups":
        """A raw integer matrix [n_part, n_hla] (or one row) of group ids 0 .. n_hla - 1, taken as it is: the levels are the
        ids as strings, an id no allele has is an empty group."""
        g = np.asarray(group_of)
        if g.ndim == 1:
            g = g.reshape(1, -1)
        if g.dtype.kind not in "iu" or g.ndim != 2 or g.shape[1] != len(alleles) or g.shape[0] < 1:
            raise ValueError(f"group_of must be an integer matrix [n_part, n_hla = {len(alleles)}], got {g.dtype} {g.shape}")
        if g.min() < 0 or g.max() >= len(alleles):
            raise ValueError(f"group ids must lie in 0 .. n_hla - 1 = {len(alleles) - 1}")
        names = [f"partition{q + 1}" for q in range(g.shape[0])] if names is None else list(names)
        return cls(alleles, names, [[str(i) for i in range(int(row.max()) + 1)] for row in g], g)

    @property
    def n_part(self) -> int:
        return len(self.names)

    @property
    def n_level(self) -> int:
        """Groups of all partitions together: the columns of the dosage output."""
        return int(sum(len(lv) for lv in self.levels))

    @property
    def offsets(self) -> np.ndarray:
        """[n_part + 1]: where each partition's groups start among the columns of the dosage output."""
        return np.concatenate([[0], np.cumsum([len(lv) for lv in self.levels], dtype=np.int64)])

    def index(self, q) -> int:
        """A partition given by its position or its name."""
        if isinstance(q, str):
            if q not in self.names:
                raise KeyError(q)
            return self.names.index(q)
        if not isinstance(q, (int, np.integer)) or isinstance(q, bool) or not (0 <= int(q) < self.n_part):
            raise IndexError(f"partition must be a name or an integer between 0 and {self.n_part - 1}: {q!r}")
        return int(q)

    def labels(self, q) -> List[str]:
        """The group name of every allele in partition q."""
        q = self.index(q)
        return [self.levels[q][g] for g in self.group_of[q]]

    def plan_for(self, model: HlaAttrBagClass) -> GroupsPlan:
        """The device plan of these partitions for ``model``, made at the first call and kept with this object (the lists
        are a sort per partition and four uploads: not something to repeat per call); plans of closed models are dropped."""
        plans = self.__dict__.setdefault("_plans", [])
        for plan in [p for p in plans if getattr(p.model, "_h", None) is None]:
            plan.close()
            plans.remove(plan)
        for plan in plans:
            if plan.model is model:
                return plan
        plans.append(GroupsPlan(model, self.group_of))
        return plans[-1]

    def __add__(self, other: "HlaAlleleGroups") -> "HlaAlleleGroups":
        if not isinstance(other, HlaAlleleGroups):
            return NotImplemented
        if other.alleles != self.alleles:
            raise ValueError("the two objects partition different allele lists")
        return HlaAlleleGroups(self.alleles, self.names + other.names, self.levels + other.levels,
                               np.concatenate([self.group_of, other.group_of]))

    def __len__(self) -> int:
        return self.n_part

    def __repr__(self):
        return f"HlaAlleleGroups({self.n_part} partitions of {len(self.alleles)} alleles, {self.n_level} groups)"


def _alleles_of(alleles) -> List[str]:
    return list(getattr(alleles, "hla_allele", alleles))


def hlaGroupsByResolution(alleles, max_resolution: str = "2-digit", rm_suffix: bool = False) -> HlaAlleleGroups:
    """The partition ``hlaAlleleDigit(alleles, max_resolution, rm_suffix)`` makes: alleles with the same shortened name are
    one group.  ``alleles``: the names, or a model."""
    alleles = _alleles_of(alleles)
    return HlaAlleleGroups.from_labels(alleles, max_resolution or "full", hlaAlleleDigit(alleles, max_resolution, rm_suffix))


def hlaGroupsByMap(alleles, mapping: Mapping[str, str], name: str) -> HlaAlleleGroups:
    """The partition a dictionary allele -> group name makes (serological groups, P / G groups, supertypes); an allele the
    dictionary does not hold keeps its own name, as ``hlaPredMerge``'s ``equivalence`` does."""
    alleles = _alleles_of(alleles)
    return HlaAlleleGroups.from_labels(alleles, name, [str(mapping.get(a, a)) for a in alleles])


def hlaGroupsBySequence(alleles, sequences: Mapping[str, str], positions: Optional[Sequence[int]] = None,
                        first: int = 1) -> HlaAlleleGroups:
    """One partition per position of an alignment: alleles with the same letter at the position are one group.
    ``sequences``: allele -> aligned string, all of one length; character i of a string is position ``first + i``.  Without
    ``positions`` every position at which the model's alleles show at least two letters gives a partition (named by the
    position); with ``positions`` exactly those do, in that order.  An allele without a sequence goes to the level ``"?"``."""
    alleles = _alleles_of(alleles)
    lengths = {len(s) for s in sequences.values()}
    if len(lengths) != 1:
        raise ValueError("the sequences must be aligned: strings of one common length")
    length = lengths.pop()
    have = [sequences.get(a) for a in alleles]
    if positions is None:
        idx = [i for i in range(length) if len({s[i] for s in have if s is not None}) >= 2]
    else:
        idx = [int(p) - int(first) for p in positions]
        if any(not (0 <= i < length) for i in idx):
            raise ValueError(f"positions must lie in {first} .. {first + length - 1}")
    if not idx:
        raise ValueError("no polymorphic position among the model's alleles")
    out = None
    for i in idx:
        one = HlaAlleleGroups.from_labels(alleles, str(int(first) + i), ["?" if s is None else s[i] for s in have])
        out = one if out is None else out + one
    return out


class HlaGroupCalls:
    """Per sample and partition the best pair of groups under the collapsed posterior: ``g1`` / ``g2`` [n_samp, n_part]
    (indices into ``groups.levels[q]``, g1 <= g2, ``NA_INTEGER`` where no pair qualifies), ``prob`` [n_samp, n_part] (the
    pair's collapsed probability), ``matching`` [n_samp], ``dosage`` [n_samp, n_level] or ``None`` with ``offsets`` (partition
    q's groups are columns ``offsets[q] : offsets[q + 1]``); ``groups``, ``locus``, ``sample_id``, ``assembly``."""

    def __init__(self, locus: str, sample_id: List, groups: HlaAlleleGroups, g1: np.ndarray, g2: np.ndarray, prob: np.ndarray,
                 matching: np.ndarray, dosage: Optional[np.ndarray] = None, assembly: str = "unknown"):
        shape = (len(sample_id), groups.n_part)
        for a in (g1, g2, prob):
            if a.shape != shape:
                raise ValueError(f"expected arrays of shape {shape}, got {a.shape}")
        if dosage is not None and dosage.shape != (len(sample_id), groups.n_level):
            raise ValueError(f"expected a dosage of shape {(len(sample_id), groups.n_level)}, got {dosage.shape}")
        self.locus, self.sample_id, self.groups, self.assembly = locus, sample_id, groups, assembly
        self.g1, self.g2, self.prob, self.matching, self.dosage = g1, g2, prob, matching, dosage
        self.offsets = groups.offsets

    def calls(self, q) -> HlaAlleleClass:
        """Partition ``q`` (its position or its name) as an :class:`HlaAlleleClass` whose alleles are the group names."""
        q = self.groups.index(q)
        return HlaAlleleClass(locus=self.locus, sample_id=list(self.sample_id), h1=np.ascontiguousarray(self.g1[:, q]),
                              h2=np.ascontiguousarray(self.g2[:, q]), levels=self.groups.levels[q],
                              prob=np.ascontiguousarray(self.prob[:, q]), matching=self.matching, assembly=self.assembly,
                              dosage=None if self.dosage is None else self.dosage_of(q))

    def dosage_of(self, q) -> np.ndarray:
        """The expected dosage of partition ``q``'s groups, [n_group, n_samp] (rows = ``groups.levels[q]``): ``hlaPredict``'s
        orientation, a view."""
        if self.dosage is None:
            raise ValueError("the call was made without dosages")
        q = self.groups.index(q)
        return self.dosage[:, int(self.offsets[q]):int(self.offsets[q + 1])].T

    def __repr__(self):
        return (f"HlaGroupCalls(locus={self.locus!r}, {len(self.sample_id)} samples, {self.groups.n_part} partitions, "
                f"{self.groups.n_level} groups, assembly={self.assembly!r})")


def hlaPredictGroups(model: HlaAttrBagClass, snp, groups: Union[HlaAlleleGroups, np.ndarray], dosage: bool = True,
                     vote: str = "prob", allele_check: bool = True, match_type: str = "Position", same_strand: bool = False,
                     verbose: bool = True, verbose_match: bool = True) -> HlaGroupCalls:
    """Per sample and partition of ``groups`` the most probable PAIR OF GROUPS under ``hlaPredict(model, snp, vote=vote)``'s
    posterior collapsed over the groups, its probability and (``dosage``) the expected dosage of every group, on the device.

    ``groups``: an :class:`HlaAlleleGroups` over the model's alleles (:func:`hlaGroupsByResolution`, :func:`hlaGroupsByMap`,
    :func:`hlaGroupsBySequence`, added up with ``+``) or an integer matrix [n_part, n_hla] of group ids; at most
    ``HIBAG_HIP_GROUPS_MAX_PART`` partitions with ``HIBAG_HIP_GROUPS_MAX_LEVELS`` groups together.  ``snp``: what
    ``hlaPredictDraws`` takes -- an :class:`HlaSNPGeno` in either memory order, a numeric matrix [n.snp, n.samp] or a vector,
    a lazily opened :class:`HlaBEDGeno`, a resident :class:`HlaDeviceCohort` --, matched as ``hlaPredict`` matches it.  With
    the identity partition the result is ``hlaPredict``'s own call, probability and dosage bit for bit."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    if not isinstance(groups, HlaAlleleGroups):
        groups = HlaAlleleGroups.from_matrix(model.obj.hla_allele, groups)
    if groups.alleles != list(model.obj.hla_allele):
        raise ValueError("'groups' partitions another allele list than the model's")
    if groups.n_part > _lib.GROUPS_MAX_PART or groups.n_level > _lib.GROUPS_MAX_LEVELS:
        raise ValueError(f"'groups' holds {groups.n_part} partitions with {groups.n_level} groups; at most {_lib.GROUPS_MAX_PART} "
                         f"(HIBAG_HIP_GROUPS_MAX_PART) with {_lib.GROUPS_MAX_LEVELS} (HIBAG_HIP_GROUPS_MAX_LEVELS)")
    vote_method = _VOTES.index(vote) + 1
    q, d = groups.n_part, groups.n_level
    what = (f"the best pair of groups in {q} partition{'s' if q > 1 else ''} of the alleles ({d} groups"
            + (", with group dosages" if dosage else "") + "), "
            + ("based on the averaged posterior probabilities" if vote_method == 1 else "by voting from all individual classifiers"))
    r = _resolve_snp(model.obj, snp, what, match_type, allele_check, same_strand, verbose, verbose_match)
    rv = _predict_resolved(model, snp, r, "groups", (groups.plan_for(model),), vote_method, want_dosage=bool(dosage))
    _warn_no_prediction(int(np.count_nonzero((rv["g1"][:, 0] == NA_INTEGER) | (rv["g2"][:, 0] == NA_INTEGER))))
    return HlaGroupCalls(locus=model.obj.hla_locus, sample_id=list(r.sample_id), groups=groups, g1=rv["g1"], g2=rv["g2"],
                         prob=rv["prob"], matching=rv["matching"], dosage=rv.get("dosage"), assembly=r.assembly)
