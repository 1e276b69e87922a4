"""``hlaPredictFamily``: children's calls weighted by their parents' posteriors, on the device.

HLA cohorts are full of trios and duos.  A child's two alleles are one allele of each parent, so the parents' SNPs say a
great deal about a child whose own SNPs are sparse -- and a caller that types every sample alone returns
Mendelian-inconsistent trios routinely.  The family finish (``hibag_hip_predict_family`` and its routes) weights every
sample's posterior with the Mendelian transmission probability its parents' results give each allele pair, divided by the
pair's prior, and calls the best pair of the weighted posterior.  The weight is built on the device from the parents'
results of the same call; 24 bytes per sample come back, plus 8 per allele with the dosages, instead of the posterior matrix
``hlaPredict(type="response+prob")`` returns for a host loop.  The result is defined exactly: a sample
without known parents gets ``hlaPredict``'s call, probability and dosage bit for bit.

Information flows DOWN only: a parent that is itself a child transmits its own weighted result, children never change their
parents' results, and siblings do not see each other.  There is no upward pass and no joint sibling calling."""

from __future__ import annotations

import sys
from typing import List, Optional, Sequence, Union

import numpy as np

from .bed import HlaBEDGeno
from .cohort import HlaDeviceCohort
from .hibag import HlaAlleleClass, HlaAttrBagClass, _predict_matrix, _resolve_snp, _warn_no_prediction
from .model import NA_INTEGER, HlaSNPGeno

_VOTES = ("prob", "majority")


def _unknown(x) -> bool:
    return x is None or (isinstance(x, float) and x != x) or (isinstance(x, str) and x.strip() in ("", "0"))


def pedigree_depth(indices: np.ndarray) -> np.ndarray:
    """depth [n] of an index pedigree int [n, 2] in ANY order: 0 without a parent among the samples, else 1 + the larger
    depth of its parents.  ``ValueError`` if somebody is their own ancestor or an index is outside -1 .. n - 1."""
    idx = np.asarray(indices)
    if idx.ndim != 2 or idx.shape[1] != 2 or idx.dtype.kind not in "iu":
        raise ValueError(f"a pedigree is an integer array [n_samp, 2], got {idx.dtype} {idx.shape}")
    n = len(idx)
    if n and (idx.min() < -1 or idx.max() >= n):
        raise ValueError("a parent index must lie in -1 .. n_samp - 1")
    # generation by generation (vectorised over the samples): a sample is ready once all its known parents are finished
    known = idx >= 0
    par = np.maximum(idx, 0)
    depth = np.zeros(n, np.int32)
    done = np.zeros(n, np.bool_)
    while not done.all():
        ready = ~done & np.all(~known | done[par], axis=1)
        if not ready.any():
            raise ValueError(f"the pedigree holds a cycle: sample {int(np.nonzero(~done)[0][0])} is its own ancestor")
        at = np.nonzero(ready)[0]
        depth[at] = np.max(np.where(known[at], depth[par[at]] + 1, 0), axis=1)
        done[at] = True
    return depth


def depth_order(indices: np.ndarray):
    """``(order, inverse, sorted_indices, depth)`` of an index pedigree in any order: ``order`` sorts the samples stably by
    depth (so parents precede their children and samples of one depth keep their order), ``inverse[order] = arange``,
    ``sorted_indices`` [n, 2] is the pedigree of the sorted samples in the sorted numbering (what the C entries take) and
    ``depth`` the depths in the CALLER's order.  A pedigree whose parents already precede their children is left as it is
    (``order`` is the identity)."""
    idx = np.ascontiguousarray(indices, np.int32)
    depth = pedigree_depth(idx)
    n = len(idx)
    if n == 0 or bool(np.all(idx < np.arange(n, dtype=np.int64)[:, None])):
        ident = np.arange(n, dtype=np.int64)
        return ident, ident, idx, depth
    order = np.argsort(depth, kind="stable")
    inverse = np.empty(n, np.int64)
    inverse[order] = np.arange(n)
    moved = idx[order]
    return order, inverse, np.where(moved >= 0, inverse[np.maximum(moved, 0)], -1).astype(np.int32), depth


class HlaPedigree:
    """A pedigree by sample id: ``sample_id``, ``father``, ``mother`` (lists of equal length; ``None``, ``""`` or ``"0"`` --
    PLINK's word -- mean unknown).  A parent need not be listed as a sample.  ``ValueError`` where an id is listed twice,
    father and mother are the same person, or somebody is their own ancestor."""

    def __init__(self, sample_id: Sequence, father: Sequence, mother: Sequence):
        self.sample_id = list(sample_id)
        self.father = [None if _unknown(f) else f for f in father]
        self.mother = [None if _unknown(m) else m for m in mother]
        if not (len(self.sample_id) == len(self.father) == len(self.mother)):
            raise ValueError("sample_id, father and mother differ in length")
        self._at = {}
        for i, sid in enumerate(self.sample_id):
            if sid in self._at:
                raise ValueError(f"sample id {sid!r} is listed twice")
            self._at[sid] = i
        for sid, f, m in zip(self.sample_id, self.father, self.mother):
            if f is not None and f == m:
                raise ValueError(f"father and mother of {sid!r} are the same person ({f!r})")
            if sid == f or sid == m:
                raise ValueError(f"{sid!r} is listed as its own parent")
        pedigree_depth(self._indices(self.sample_id, self._at))          # (raises on a cycle)

    def _indices(self, ids: Sequence, at: dict) -> np.ndarray:
        out = np.full((len(ids), 2), -1, np.int32)
        for i, sid in enumerate(ids):
            j = self._at.get(sid)
            if j is None:
                continue
            out[i, 0] = at.get(self.father[j], -1) if self.father[j] is not None else -1
            out[i, 1] = at.get(self.mother[j], -1) if self.mother[j] is not None else -1
        return out

    def indices_for(self, sample_ids: Sequence) -> np.ndarray:
        """int32 [n, 2]: (father, mother) of every sample of ``sample_ids`` as indices into ``sample_ids``; -1 for an unknown
        parent, a parent absent from ``sample_ids`` and a sample this pedigree does not list."""
        ids = list(sample_ids)
        at = {}
        for i, sid in enumerate(ids):
            at.setdefault(sid, i)
        return self._indices(ids, at)

    def __len__(self) -> int:
        return len(self.sample_id)

    def __repr__(self):
        both = sum(1 for f, m in zip(self.father, self.mother) if f is not None and m is not None)
        one = sum(1 for f, m in zip(self.father, self.mother) if (f is None) != (m is None))
        return f"HlaPedigree({len(self)} samples: {both} with two parents, {one} with one)"


def hlaPedigreeFromFam(path: str) -> HlaPedigree:
    """The pedigree of a PLINK ``.fam`` file: columns 2-4 (individual, father, mother; ``0`` = unknown)."""
    ids, fa, mo = [], [], []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) < 4:
                raise ValueError(f"{path}: a .fam line holds at least four columns: {line!r}")
            ids.append(t[1]); fa.append(t[2]); mo.append(t[3])
    return HlaPedigree(ids, fa, mo)


def hlaModelAllelePrior(model) -> np.ndarray:
    """The allele prior the model's classifiers actually carry: q[h] = the mean over the classifiers of the summed
    haplotype frequencies of allele h.  An allele no classifier holds (q = 0) gets 1.0: its posterior is 0 anyway.  (The
    model object's ``hla_freq`` is the training cohort's and need not agree with it.)"""
    obj = getattr(model, "obj", model)
    n = int(obj.n_hla)
    q = np.zeros(n, np.float64)
    for c in obj.classifiers:
        q += np.bincount(np.asarray(c.hla, np.int64), weights=np.asarray(c.freq, np.float64), minlength=n)
    if len(obj.classifiers):
        q /= len(obj.classifiers)
    return np.where(q > 0, q, 1.0)


class HlaFamilyCalls:
    """Per sample the best allele pair under its posterior weighted by its parents' results: ``h1`` / ``h2`` [n_samp]
    (0-based indices into ``alleles``, h1 <= h2, ``NA_INTEGER`` where no pair qualifies), ``prob`` (CONDITIONAL on the
    family: ``prob_joint / support`` where ``support > 0``, the joint value as it is elsewhere), ``prob_joint``, ``support``
    (the weighted mass of all pairs: a Bayes-factor-like family fit, well below 1 where the child's own SNPs contradict its
    parents), ``matching``, ``dosage`` [n_hla, n_samp] or ``None`` (conditional in the same way), ``pedigree`` int32
    [n_samp, 2] (indices into the samples, -1 = unknown) and ``depth`` [n_samp]; ``locus``, ``sample_id``, ``assembly``.
    All in the caller's sample order."""

    def __init__(self, locus: str, sample_id: List, alleles: Sequence[str], h1: np.ndarray, h2: np.ndarray,
                 prob_joint: np.ndarray, support: np.ndarray, matching: np.ndarray, dosage_joint: Optional[np.ndarray],
                 pedigree: np.ndarray, depth: np.ndarray, assembly: str = "unknown"):
        self.locus, self.sample_id, self.alleles, self.assembly = locus, sample_id, list(alleles), assembly
        self.h1, self.h2, self.prob_joint, self.support, self.matching = h1, h2, prob_joint, support, matching
        self.pedigree, self.depth = pedigree, depth
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
        return f"HlaFamilyCalls(locus={self.locus!r}, {len(self.sample_id)} samples, assembly={self.assembly!r})"


def _indices_of(pedigree, snp, sample_id: Sequence, n_samp: int) -> np.ndarray:
    if isinstance(pedigree, HlaPedigree):
        if not isinstance(snp, HlaSNPGeno):
            raise TypeError("an HlaPedigree is matched by sample id: 'snp' must be an HlaSNPGeno (a numeric matrix takes the "
                            "pedigree as an integer array [n_samp, 2])")
        return pedigree.indices_for(list(sample_id))
    idx = np.asarray(pedigree)
    if idx.dtype.kind not in "iu" or idx.ndim != 2 or idx.shape[1] != 2:
        raise TypeError("'pedigree' must be an HlaPedigree or an integer array [n_samp, 2] of (father, mother) sample indices")
    if idx.shape[0] != n_samp:
        raise ValueError(f"'pedigree' holds {idx.shape[0]} samples, 'snp' {n_samp}")
    return np.ascontiguousarray(idx, np.int32)


def _gather_columns(mat: np.ndarray, order: np.ndarray) -> np.ndarray:
    """Columns ``order`` of the matrix [SNP, sample], gathered once, in the memory order it came in."""
    if mat.flags.f_contiguous and not mat.flags.c_contiguous:
        return mat.T[order].T
    return np.ascontiguousarray(mat[:, order])


def hlaPredictFamily(model: HlaAttrBagClass, snp, pedigree: Union[HlaPedigree, np.ndarray], prior="model", dosage: bool = False,
                     vote: str = "prob", allele_check: bool = True, match_type: str = "Position", same_strand: bool = False,
                     verbose: bool = True, verbose_match: bool = True) -> HlaFamilyCalls:
    """Per sample the most probable allele pair under ``hlaPredict(model, snp, vote=vote)``'s posterior WEIGHTED by the
    Mendelian transmission probability its parents' results give each pair, on the device.

    ``pedigree``: an :class:`HlaPedigree` (matched to the samples of an :class:`HlaSNPGeno` by id; parents absent from the
    genotypes are unknown) or an integer array [n_samp, 2] of (father, mother) as indices into the samples of ``snp``, -1 for
    unknown.  ``prior``: ``"model"`` (:func:`hlaModelAllelePrior`: the prior the classifiers carry), ``None`` (no division)
    or an array over the model's alleles, every entry finite and > 0.  ``snp``: an :class:`HlaSNPGeno` in either memory
    order, a numeric matrix [n.snp, n.samp] or a vector, matched as ``hlaPredict`` matches it.  Where the samples' order
    does not already put parents before their children they are sorted stably by depth -- one gather of the columns -- and
    every output comes back in the caller's order.  A lazily opened :class:`HlaBEDGeno` or a resident
    :class:`HlaDeviceCohort` is refused (their sample order is the file's): read the genotypes with ``hlaBED2Geno``.

    Information flows down only: parents' results are ``hlaPredict``'s own unless they are children themselves; children do
    not change their parents' results and siblings do not see each other."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if isinstance(snp, (HlaBEDGeno, HlaDeviceCohort)):
        raise TypeError(f"hlaPredictFamily orders the samples so that parents precede their children, which a {type(snp).__name__} "
                        "cannot: read the genotypes into memory with hlaBED2Geno(...) and pass that")
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    vote_method = _VOTES.index(vote) + 1
    if isinstance(prior, str):
        if prior != "model":
            raise ValueError("'prior' should be \"model\", None or an array over the model's alleles")
        q = model.__dict__.get("_allele_prior")              # (made once per model)
        if q is None:
            q = model.__dict__["_allele_prior"] = hlaModelAllelePrior(model)
    elif prior is None:
        q = None
    else:
        q = np.ascontiguousarray(prior, np.float64)
        if q.shape != (int(model.obj.n_hla),):
            raise ValueError(f"'prior' must hold one entry per allele of the model ({int(model.obj.n_hla)}), got {q.shape}")
        if not np.all(np.isfinite(q) & (q > 0)):
            raise ValueError("every entry of 'prior' must be finite and > 0")
    what = ("the best allele pair under the posterior weighted by the parents' posteriors" + (", with conditional dosages" if dosage else "")
            + ", " + ("based on the averaged posterior probabilities" if vote_method == 1 else "by voting from all individual classifiers"))
    r = _resolve_snp(model.obj, snp, what, match_type, allele_check, same_strand, verbose, verbose_match)
    idx = _indices_of(pedigree, snp, r.sample_id, r.n_samp)
    if np.any((idx[:, 0] >= 0) & (idx[:, 0] == idx[:, 1])):
        raise ValueError("father and mother of a sample are the same person")
    order, inverse, sorted_idx, depth = depth_order(idx)
    if verbose:
        known = np.count_nonzero(idx >= 0, axis=1)
        print(f"Pedigree: {int(np.count_nonzero(known == 2))} trios, {int(np.count_nonzero(known == 1))} duos, "
              f"{int(np.count_nonzero(known == 0))} founders; deepest generation {int(depth.max()) if len(depth) else 0}", file=sys.stdout)
    moved = not np.array_equal(order, np.arange(len(order)))
    mat = _gather_columns(r.mat, order) if moved else r.mat
    rv = _predict_matrix(model, "family", mat, r.sel, r.flip, (sorted_idx, q), vote_method, want_dosage=bool(dosage))
    if moved:
        rv = {k: v[inverse] for k, v in rv.items()}
    _warn_no_prediction(int(np.count_nonzero((rv["h1"] == NA_INTEGER) | (rv["h2"] == NA_INTEGER))))
    return HlaFamilyCalls(locus=model.obj.hla_locus, sample_id=list(r.sample_id), alleles=model.obj.hla_allele, h1=rv["h1"],
                          h2=rv["h2"], prob_joint=rv["prob"], support=rv["support"], matching=rv["matching"],
                          dosage_joint=rv.get("dosage"), pedigree=idx, depth=depth, assembly=r.assembly)


class HlaMendelCheck:
    """What :func:`hlaMendelCheck` found: ``child`` (indices of the children checked: called themselves, with at least one
    called parent among the samples), ``consistent`` (bool per checked child), ``n_parents`` (1 or 2 per checked child);
    ``n_checked``, ``n_inconsistent`` and ``n_inconsistent_trios`` (among the children with two called parents)."""

    def __init__(self, child: np.ndarray, consistent: np.ndarray, n_parents: np.ndarray):
        self.child, self.consistent, self.n_parents = child, consistent, n_parents
        self.n_checked = int(len(child))
        self.n_inconsistent = int(np.count_nonzero(~consistent))
        self.n_inconsistent_trios = int(np.count_nonzero(~consistent & (n_parents == 2)))

    def __repr__(self):
        return (f"HlaMendelCheck({self.n_checked} children checked, {self.n_inconsistent} Mendelian-inconsistent, "
                f"{self.n_inconsistent_trios} of them with both parents typed)")


def hlaMendelCheck(hla, pedigree: Union[HlaPedigree, np.ndarray]) -> HlaMendelCheck:
    """Whether the called allele pairs are Mendelian-consistent, per child with at least one typed parent.  ``hla``: an
    :class:`HlaAlleleClass` (``hlaPredict``'s value) or an :class:`HlaFamilyCalls`; ``pedigree``: an :class:`HlaPedigree`
    (matched by ``hla.sample_id``) or an integer array [n_samp, 2].  A trio is consistent when one of the child's alleles is
    among the father's two and the other among the mother's; a duo when one of the child's alleles is among the parent's.
    Samples and parents without a call are not counted."""
    if isinstance(hla, HlaFamilyCalls):
        hla = hla.calls()
    a1, a2 = list(hla.allele1), list(hla.allele2)
    n = len(a1)
    idx = pedigree.indices_for(list(hla.sample_id)) if isinstance(pedigree, HlaPedigree) else np.asarray(pedigree)
    if idx.shape != (n, 2):
        raise ValueError(f"the pedigree holds {idx.shape[0]} samples, the calls {n}")
    called = [a1[i] is not None and a2[i] is not None for i in range(n)]
    child, ok, cnt = [], [], []
    for s in range(n):
        if not called[s]:
            continue
        par = [int(p) for p in idx[s] if p >= 0 and called[int(p)]]
        if not par:
            continue
        sets = [(a1[p], a2[p]) for p in par]
        if len(par) == 2:
            good = (a1[s] in sets[0] and a2[s] in sets[1]) or (a2[s] in sets[0] and a1[s] in sets[1])
        else:
            good = a1[s] in sets[0] or a2[s] in sets[0]
        child.append(s); ok.append(good); cnt.append(len(par))
    return HlaMendelCheck(np.array(child, np.int64), np.array(ok, np.bool_), np.array(cnt, np.int64))
