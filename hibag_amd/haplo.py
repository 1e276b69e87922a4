"""``hlaHaplotypes``: which alleles of several HLA loci sit together on a chromosome -- A*01:01~B*08:01~DRB1*03:01 and its
frequency -- from the per-locus calls of one cohort, by an EM over the haplotype pairs the calls allow, on the device.

Per sample and locus the input is a list of candidate allele pairs with weights: the k best pairs of ``hlaPredictTopK``
(an :class:`HlaTopCalls`), or one certain pair (an :class:`HlaAlleleClass` from ``hlaPredict`` or from lab typing).  A STATE
of a sample is a candidate per locus and a phase; the EM estimates the haplotype frequencies that make the cohort's states
most likely, and each sample's most probable state under them is its jointly informed call: linkage disequilibrium lets
one locus's uncertain call lean on the others.  The host half here gathers and trims the candidates; the states, the
haplotype dictionary, the iterations and the calls are ``hibag_hip_haplo_*`` (kernels: ``csrc/hibag_k_haplo.h``).  Every
number is defined operation by operation in DESIGN.md section 29, and ``tests/haplo_reference.py`` restates it in numpy.

Not built: division by the per-locus model prior; marginalising a sample's missing locus over all alleles (the sample is
left out); more than 6 loci; progressive insertion or trimming of the dictionary; ``hlaPredictLoci(type="topk")`` as a
source.  (Association tests on haplotypes: ``hlaAssocHaplo``, from ``dosage`` or ``as_alleles`` of the result here.)"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .hibag import HlaAlleleClass
from .model import NA_INTEGER
from .topk import HlaTopCalls

MAX_LOCI = 6            # HIBAG_HIP_HAPLO_MAX_LOCI
MAX_ALLELE = 1024       # HIBAG_HIP_HAPLO_MAX_ALLELE
MAX_K = 64              # HIBAG_HIP_HAPLO_MAX_K
KEY_BITS = 10
MAX_ENTRIES = 2 ** 31 - 1


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def state_count(n_hom, n_het):
    """States of a sample with ``n_hom[l]`` homozygous and ``n_het[l]`` heterozygous candidates at locus l (the last axis):
    ``(prod (hom + 2 het) + prod hom) / 2`` -- every ordered haplotype pair counted once and the all-homozygous ones, which
    are their own mirror image, added before halving."""
    n_hom, n_het = np.asarray(n_hom, np.int64), np.asarray(n_het, np.int64)
    return (np.prod(n_hom + 2 * n_het, axis=-1) + np.prod(n_hom, axis=-1)) // 2


def _one_locus(res) -> Tuple[str, list, List, np.ndarray, np.ndarray, np.ndarray]:
    """(locus, levels, sample ids, h1, h2, prob [n, k]) of one result."""
    if isinstance(res, HlaTopCalls):
        return res.locus, list(res.levels), list(res.sample_id), res.h1, res.h2, res.prob
    if isinstance(res, HlaAlleleClass):
        n = len(res.sample_id)
        if res.h1 is not None and res.h2 is not None and res._levels is not None:
            levels, h1, h2 = list(res._levels), np.asarray(res.h1, np.int32), np.asarray(res.h2, np.int32)
        else:                          # names only (hlaAllele): the levels are the names in order
            a1, a2 = list(res.allele1), list(res.allele2)
            levels = sorted({a for a in a1 + a2 if a is not None})
            at = {a: i for i, a in enumerate(levels)}
            h1 = np.array([NA_INTEGER if a is None else at[a] for a in a1], np.int32)
            h2 = np.array([NA_INTEGER if a is None else at[a] for a in a2], np.int32)
        return res.locus, levels, list(res.sample_id), h1.reshape(n, 1), h2.reshape(n, 1), np.ones((n, 1), np.float64)
    raise TypeError("every entry of 'calls' must be an HlaTopCalls or an HlaAlleleClass")


def gather_candidates(calls) -> Tuple[List[str], List[list], List, np.ndarray, np.ndarray, np.ndarray]:
    """``calls`` as (loci, levels per locus, sample ids, h1, h2, prob [L, n, k]): the samples of the first result, in its
    order, matched by id; per sample and locus the candidates in rank order at the front, h1 <= h2, ``NA_INTEGER`` / 0.0 behind
    them.  NA ranks and ranks with probability 0 are no candidates."""
    if isinstance(calls, Mapping):
        names, results = [str(k) for k in calls.keys()], list(calls.values())
    elif isinstance(calls, (list, tuple)):
        names, results = None, list(calls)
    else:
        raise TypeError("'calls' must be a mapping {locus: result} or a sequence of results")
    if not (2 <= len(results) <= MAX_LOCI):
        raise ValueError(f"hlaHaplotypes needs 2 .. {MAX_LOCI} loci, got {len(results)}")
    parts = [_one_locus(r) for r in results]
    loci = names if names is not None else [p[0] for p in parts]
    ids = parts[0][2]
    n, k = len(ids), max(p[3].shape[1] for p in parts)
    if len(set(ids)) != n:
        raise ValueError("the sample ids of the first result are not unique")
    if k > MAX_K:
        raise ValueError(f"at most {MAX_K} candidates per sample and locus, got {k}")
    h1 = np.full((len(parts), n, k), NA_INTEGER, np.int32)
    h2 = np.full((len(parts), n, k), NA_INTEGER, np.int32)
    prob = np.zeros((len(parts), n, k), np.float64)
    for l, (_, levels, sid, a, b, p) in enumerate(parts):
        if len(levels) > MAX_ALLELE:
            raise ValueError(f"locus {loci[l]} has {len(levels)} alleles; at most {MAX_ALLELE}")
        if l == 0:
            rows = np.arange(n)
        else:
            at = {s: i for i, s in enumerate(sid)}
            missing = [s for s in ids if s not in at]
            if missing:
                raise ValueError(f"{len(missing)} sample ids of the first result are missing from locus {loci[l]}: {missing[:5]}")
            rows = np.array([at[s] for s in ids], np.int64)
        a, b, p = np.asarray(a)[rows], np.asarray(b)[rows], np.asarray(p, np.float64)[rows]
        if np.isnan(p).any() or (p < 0).any() or np.isinf(p).any():
            raise ValueError(f"locus {loci[l]} has probabilities that are negative or not finite")
        ok = (a != NA_INTEGER) & (b != NA_INTEGER) & (p > 0)
        if ((a[ok] < 0) | (b[ok] < 0) | (a[ok] >= len(levels)) | (b[ok] >= len(levels))).any():
            raise ValueError(f"locus {loci[l]} has allele indices outside its {len(levels)} levels")
        order = np.argsort(~ok, axis=1, kind="stable")                # the candidates to the front, rank order kept
        ok_s = np.take_along_axis(ok, order, 1)
        kk = a.shape[1]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        h1[l, :, :kk] = np.where(ok_s, np.take_along_axis(lo, order, 1), NA_INTEGER)
        h2[l, :, :kk] = np.where(ok_s, np.take_along_axis(hi, order, 1), NA_INTEGER)
        prob[l, :, :kk] = np.where(ok_s, np.take_along_axis(p, order, 1), 0.0)
    return loci, [p[1] for p in parts], ids, h1, h2, prob


def trim_candidates(h1: np.ndarray, h2: np.ndarray, prob: np.ndarray, min_prob: float, max_states: int,
                    sample_id: Optional[Sequence] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The host's trimming of gathered candidates [L, n, k]: every candidate of rank >= 1 with
    ``p < min_prob`` goes; then, while a sample has more than ``max_states`` states, its remaining candidate of rank >= 1
    with the smallest p goes, of equals the one at the highest locus, then of the highest rank.  Rank 0 stays; a sample
    whose rank-0 candidates alone exceed the cap is a ``ValueError``.  Returns the trimmed arrays (candidates at the front)
    and ``n_trimmed`` [n]."""
    L, n, k = h1.shape
    keep = h1 != NA_INTEGER
    rank = np.arange(k)[None, None, :]
    keep_min = keep & ((rank == 0) | (prob >= min_prob))
    het = h1 != h2
    over = np.flatnonzero(state_count((keep_min & ~het).sum(axis=2).T, (keep_min & het).sum(axis=2).T) > max_states)
    for s in over:                                   # (rare: one sample at a time)
        m = keep_min[:, s, :]                        # a view: what goes here is gone below
        count = lambda: int(state_count((m & ~het[:, s, :]).sum(axis=1), (m & het[:, s, :]).sum(axis=1)))      # noqa: E731
        while count() > max_states:
            cand = [(prob[l, s, r], -l, -r) for l in range(L) for r in range(1, k) if m[l, r]]
            if not cand:
                who = s if sample_id is None else sample_id[s]
                raise ValueError(f"sample {who!r} has {count()} states with its first candidates alone, "
                                 f"more than max_states = {max_states}")
            _, nl, nr = min(cand)
            m[-nl, -nr] = False
    n_trimmed = (keep & ~keep_min).sum(axis=(0, 2)).astype(np.int32)
    order = np.argsort(~keep_min, axis=2, kind="stable")
    ok = np.take_along_axis(keep_min, order, 2)
    return (np.where(ok, np.take_along_axis(h1, order, 2), NA_INTEGER).astype(np.int32),
            np.where(ok, np.take_along_axis(h2, order, 2), NA_INTEGER).astype(np.int32),
            np.where(ok, np.take_along_axis(prob, order, 2), 0.0), n_trimmed)


class _DeviceHaplo:
    """The states and the dictionary of one cohort on the device (``hibag_hip_haplo``): candidates [L, n, k] as
    ``trim_candidates`` returns them."""

    def __init__(self, h1: np.ndarray, h2: np.ndarray, prob: np.ndarray, max_states: int, device: int = -1):
        h1, h2 = np.ascontiguousarray(h1, np.int32), np.ascontiguousarray(h2, np.int32)
        prob = np.ascontiguousarray(prob, np.float64)
        if h1.ndim != 3 or h1.shape != h2.shape or h1.shape != prob.shape:
            raise ValueError("h1, h2 and prob must be [loci, samples, k] arrays of one shape")
        self.n_loci, self.n_samp, self.k = h1.shape
        lib = _lib.lib()
        self._h = lib.hibag_hip_haplo_new(self.n_samp, self.n_loci, self.k, _ptr(h1), _ptr(h2), _ptr(prob), int(max_states), int(device))
        if not self._h:
            raise _lib.HibagHipError(-1, lib.hibag_hip_last_error().decode("utf-8", "replace"))
        n_hap, n_states, n_used = C.c_int32(), C.c_int64(), C.c_int32()
        used, states = np.empty(self.n_samp, np.int32), np.empty(self.n_samp, np.int64)
        _lib.check(lib.hibag_hip_haplo_dims(self._h, C.byref(n_hap), C.byref(n_states), C.byref(n_used), _ptr(used), _ptr(states)))
        self.n_hap, self.n_states, self.n_used = n_hap.value, n_states.value, n_used.value
        self.used, self.states = used.astype(bool), states

    def close(self) -> None:
        if self._h:
            _lib.lib().hibag_hip_haplo_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def fit(self, maxit: int, tol: float) -> Dict[str, object]:
        """freq, keys [H] in ascending key order; n_iter, delta, n_zero."""
        freq, keys = np.empty(self.n_hap, np.float64), np.empty(self.n_hap, np.uint64)
        n_iter, delta, n_zero = C.c_int32(), C.c_double(), C.c_int32()
        _lib.check(_lib.lib().hibag_hip_haplo_fit(self._h, int(maxit), float(tol), _ptr(freq), _ptr(keys), C.byref(n_iter), C.byref(delta),
                                                  C.byref(n_zero)))
        return dict(freq=freq, keys=keys, n_iter=n_iter.value, delta=delta.value, n_zero=n_zero.value)

    def calls(self) -> Dict[str, np.ndarray]:
        """hapA, hapB [n, L], prob, total [n] under the last fit."""
        a, b = np.empty((self.n_samp, self.n_loci), np.int32), np.empty((self.n_samp, self.n_loci), np.int32)
        prob, total = np.empty(self.n_samp, np.float64), np.empty(self.n_samp, np.float64)
        _lib.check(_lib.lib().hibag_hip_haplo_calls(self._h, _ptr(a), _ptr(b), _ptr(prob), _ptr(total)))
        return dict(hapA=a, hapB=b, prob=prob, total=total)

    def dosage(self, hap: Sequence[int]) -> np.ndarray:
        """float64 [m, n] under the last fit: every sample's expected copies of the haplotypes ``hap`` (indices into the fit's
        ascending-key order), NaN for a sample left out."""
        hap = np.ascontiguousarray(hap, np.int32)
        out = np.empty((len(hap), self.n_samp), np.float64)
        _lib.check(_lib.lib().hibag_hip_haplo_dosage(self._h, _ptr(hap), len(hap), _ptr(out)))
        return out


def decode_keys(keys: np.ndarray, n_loci: int) -> np.ndarray:
    """int32 [H, L]: the allele index of every locus of every key."""
    keys = np.asarray(keys, np.uint64)
    return np.stack([((keys >> np.uint64(KEY_BITS * l)) & np.uint64(MAX_ALLELE - 1)).astype(np.int32) for l in range(n_loci)], axis=1)


class HlaHaplotypeResult:
    """What ``hlaHaplotypes`` returns.

    ``loci``, ``levels`` (allele names per locus); ``haplotypes`` int32 [H, L] (allele indices per locus) with ``freq`` [H],
    sorted by frequency descending, equal frequencies by ascending key (``keys``); ``n_iter``, ``converged``, ``delta``
    (the last iteration's largest frequency change), ``loglik`` (the sum of log ``total`` over the used samples with a
    total above 0; ``n_zero`` samples have total 0).  Per sample, in ``sample_id`` order: ``h1`` / ``h2`` int32 [n, L] (the two
    haplotypes of the most probable state, ``NA_INTEGER`` for a sample left out), ``prob`` (that state's posterior), ``used``,
    ``total`` (the sample's likelihood), ``n_states``, ``n_trimmed`` (candidates the trimming dropped).  With
    ``dosage_min_freq``: ``dosage_index`` (the positions in ``haplotypes`` with ``freq >= dosage_min_freq``, in order) and
    ``dosage`` float64 [m, n], every sample's expected number of copies of those haplotypes under its posterior over its
    states (NaN for a sample left out); else both are ``None``."""

    dosage_min_freq: Optional[float] = None
    dosage_index: Optional[np.ndarray] = None
    dosage: Optional[np.ndarray] = None

    def __init__(self, loci, levels, sample_id, haplotypes, freq, keys, n_iter, converged, delta, loglik, n_zero, h1, h2, prob, used,
                 total, n_states, n_trimmed, rank0):
        self.loci, self.levels, self.sample_id = list(loci), [list(v) for v in levels], list(sample_id)
        self.haplotypes, self.freq, self.keys = haplotypes, freq, keys
        self.n_iter, self.converged, self.delta, self.loglik, self.n_zero = n_iter, converged, delta, loglik, n_zero
        self.h1, self.h2, self.prob, self.used, self.total = h1, h2, prob, used, total
        self.n_states, self.n_trimmed = n_states, n_trimmed
        self._rank0 = rank0                          # (lo, hi) int32 [L, n] of every locus's first candidate

    @property
    def n_used(self) -> int:
        return int(np.count_nonzero(self.used))

    def names(self, i: int) -> str:
        """Haplotype i as allele names joined with ``~``."""
        return "~".join(str(self.levels[l][int(a)]) for l, a in enumerate(self.haplotypes[i]))

    def _locus(self, locus) -> int:
        if isinstance(locus, (int, np.integer)) and not isinstance(locus, bool):
            if not (0 <= int(locus) < len(self.loci)):
                raise IndexError(f"locus index {locus} outside 0 .. {len(self.loci) - 1}")
            return int(locus)
        if locus not in self.loci:
            raise KeyError(f"no locus {locus!r}; the loci are {self.loci}")
        return self.loci.index(locus)

    def locus_calls(self, locus) -> HlaAlleleClass:
        """The jointly informed calls at one locus (a name or an index): the two alleles of the sample's haplotype pair, the
        smaller index first; ``prob`` is the posterior of the whole multi-locus state."""
        l = self._locus(locus)
        a, b = self.h1[:, l], self.h2[:, l]
        na = ~self.used
        lo, hi = np.where(na, NA_INTEGER, np.minimum(a, b)).astype(np.int32), np.where(na, NA_INTEGER, np.maximum(a, b)).astype(np.int32)
        return HlaAlleleClass(locus=self.loci[l], sample_id=list(self.sample_id), h1=lo, h2=hi, levels=self.levels[l],
                              prob=self.prob.copy())

    def as_alleles(self, min_freq: float = 0.0) -> HlaAlleleClass:
        """The called haplotype pairs as an :class:`HlaAlleleClass` whose "alleles" are haplotypes: the levels are the names
        of the haplotypes with ``freq >= min_freq``, in result order, and ``"rare"`` for every other one; NA for a sample left
        out; ``prob`` is the called state's posterior.  With it the association entries run on best-guess haplotypes as they
        are."""
        if not (isinstance(min_freq, (int, float, np.floating)) and not isinstance(min_freq, bool) and 0 <= float(min_freq) <= 1):
            raise ValueError("min_freq must be a number in [0, 1]")
        sel = np.flatnonzero(self.freq >= float(min_freq))
        levels = [self.names(int(i)) for i in sel] + ["rare"]
        sel_keys = np.asarray(self.keys, np.uint64)[sel]
        by_key = np.argsort(sel_keys, kind="stable")
        shift = (KEY_BITS * np.arange(len(self.loci))).astype(np.uint64)
        used = np.asarray(self.used, bool)

        def index(h):
            key = (np.where(used[:, None], h, 0).astype(np.uint64) << shift[None, :]).sum(axis=1, dtype=np.uint64)
            pos = np.minimum(np.searchsorted(sel_keys[by_key], key), max(len(sel) - 1, 0))
            hit = (sel_keys[by_key][pos] == key) if len(sel) else np.zeros(len(key), bool)
            out = np.where(hit, by_key[pos] if len(sel) else 0, len(sel))
            return np.where(used, out, NA_INTEGER).astype(np.int32)

        return HlaAlleleClass(locus="~".join(self.loci), sample_id=list(self.sample_id), h1=index(self.h1), h2=index(self.h2), levels=levels,
                              prob=self.prob.copy())

    @property
    def n_changed(self) -> np.ndarray:
        """Per locus: the used samples whose pair differs from their first candidate."""
        out = np.zeros(len(self.loci), np.int64)
        for l in range(len(self.loci)):
            lo, hi = np.minimum(self.h1[:, l], self.h2[:, l]), np.maximum(self.h1[:, l], self.h2[:, l])
            out[l] = np.count_nonzero(self.used & ((lo != self._rank0[0][l]) | (hi != self._rank0[1][l])))
        return out

    def __repr__(self):
        return (f"HlaHaplotypeResult({'~'.join(self.loci)}: {len(self.freq)} haplotypes, {self.n_used} of {len(self.sample_id)} samples, "
                f"{self.n_iter} iterations, converged={self.converged})")


def hlaHaplotypes(calls: Union[Mapping, Sequence], max_states: int = 4096, min_prob: float = 0.01, maxit: int = 200,
                  tol: float = 1e-8, verbose: bool = True, dosage_min_freq: Optional[float] = None) -> HlaHaplotypeResult:
    """Haplotype frequencies over the loci of ``calls`` and every sample's most probable haplotype pair.

    ``calls``: a mapping ``{locus: result}`` or a sequence of results, 2 .. 6 loci, each an :class:`HlaTopCalls` (k candidates
    with ``prob``; NA ranks and ranks with probability 0 are ignored) or an :class:`HlaAlleleClass` (one pair, weight 1).
    Samples are matched by ``sample_id`` in the order of the first result; an id missing from another result is a
    ``ValueError``.  A sample without a candidate at some locus is left out (``used`` False).  Candidates of rank >= 1 below
    ``min_prob`` are dropped, then the least probable ones until the sample has at most ``max_states`` states.  The EM starts
    from equal frequencies and stops after the first iteration whose largest frequency change is at most ``tol``, or after
    ``maxit`` iterations.  ``dosage_min_freq``: also return every sample's expected dosage of the haplotypes with at least
    that frequency (``dosage_index``, ``dosage`` of the result) -- what ``hlaAssocHaplo`` tests."""
    if dosage_min_freq is not None and not (isinstance(dosage_min_freq, (int, float, np.floating)) and not isinstance(dosage_min_freq, bool)
                                            and 0 <= float(dosage_min_freq) <= 1):
        raise ValueError("dosage_min_freq must be None or a number in [0, 1]")
    if not isinstance(max_states, (int, np.integer)) or isinstance(max_states, bool) or not (1 <= int(max_states) <= MAX_ENTRIES // 2):
        raise ValueError("max_states must be an integer between 1 and 2^30 - 1")
    if not isinstance(maxit, (int, np.integer)) or isinstance(maxit, bool) or int(maxit) < 1:
        raise ValueError("maxit must be an integer >= 1")
    if not (isinstance(tol, (int, float, np.floating)) and float(tol) >= 0):
        raise ValueError("tol must be a number >= 0")
    if not (isinstance(min_prob, (int, float, np.floating)) and 0 <= float(min_prob) <= 1):
        raise ValueError("min_prob must be a number in [0, 1]")
    loci, levels, ids, h1, h2, prob = gather_candidates(calls)
    rank0 = (h1[:, :, 0].copy(), h2[:, :, 0].copy())
    h1, h2, prob, n_trimmed = trim_candidates(h1, h2, prob, float(min_prob), int(max_states), ids)
    has = (h1 != NA_INTEGER).any(axis=2).all(axis=0)
    if not has.any():
        raise ValueError("no sample has a candidate at every locus")
    het = h1 != h2
    n_cand = h1 != NA_INTEGER
    per = state_count((n_cand & ~het).sum(axis=2).T, (n_cand & het).sum(axis=2).T)
    if 2 * int(per[has].sum()) > MAX_ENTRIES:
        raise ValueError(f"{int(per[has].sum())} states in total: more than 2^31 - 1 entries (two per state); lower max_states or raise min_prob")
    with _DeviceHaplo(h1, h2, prob, int(max_states)) as dev:
        if verbose:
            print(f"hlaHaplotypes: {len(loci)} loci ({', '.join(loci)}), {dev.n_used} of {len(ids)} samples used, "
                  f"{dev.n_states} states, {dev.n_hap} haplotypes")
        fit = dev.fit(int(maxit), float(tol))
        got = dev.calls()
        used, states = dev.used, dev.states
        order = np.lexsort((fit["keys"], -fit["freq"]))                # frequency descending, then key ascending
        dosage_index = dosage = None
        if dosage_min_freq is not None:
            dosage_index = np.flatnonzero(fit["freq"][order] >= float(dosage_min_freq))
            dosage = dev.dosage(order[dosage_index]) if len(dosage_index) else np.zeros((0, len(ids)))
    converged = bool(fit["delta"] <= float(tol))
    tot = got["total"][used]
    loglik = float(sum(math.log(t) for t in tot if t > 0))
    if verbose:
        print(f"  {fit['n_iter']} iterations, delta = {fit['delta']:.3g}" + ("" if converged else " (not converged)") +
              f", log-likelihood {loglik:.6f}" + (f", {fit['n_zero']} samples with likelihood 0" if fit["n_zero"] else ""))
    n_trimmed = np.where(used, n_trimmed, 0).astype(np.int32)
    res = HlaHaplotypeResult(loci, levels, ids, decode_keys(fit["keys"][order], len(loci)), fit["freq"][order], fit["keys"][order],
                             fit["n_iter"], converged, fit["delta"], loglik, fit["n_zero"], got["hapA"], got["hapB"], got["prob"],
                             used, got["total"], states, n_trimmed, rank0)
    if dosage_min_freq is not None:
        res.dosage_min_freq, res.dosage_index, res.dosage = float(dosage_min_freq), dosage_index, dosage
    return res
