"""``hlaPredictMerge``: one cohort typed with several models of one locus (per ancestry, per SNP array) and the
predictions merged -- ``hlaPredMerge(hlaPredict(m1, snp, type="response+prob"), hlaPredict(m2, snp, ...), ...)`` in one
call whose posterior matrices never leave the device.

The names are settled on the host (:func:`hibag_amd.merge.merge_plan`), the SNP matching per model is ``hlaPredict``'s own
(``plan_snps_for_predict``), and ``hibag_hip_predict_merge`` does the rest: cohort up once, per chunk of samples the k
predictions and the merge behind them on one stream, the requested outputs down.  Bit-identical to the composed route
(the one documented exception is the dosage of a ONE-sample cohort, where ``hlaPredMerge``'s numpy sum
is pairwise and the device keeps the reference's row order).

Unlike the composed route the call does not warn about samples a single model could not predict: the per-model calls are
not formed.
"""

from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _lib
from . import hibag as _hb
from .bed import HlaBEDGeno
from .hibag import HlaAlleleClass, HlaAttrBagClass, _as_integer, _as_ptr
from .merge import MergePlan, hlaAlleleDigit, merge_plan
from .model import HlaSNPGeno

MAX_MODELS = 16          # HIBAG_MERGE_MAX_MODELS of the library: the sources travel as kernel arguments


def _merge_weights(weight, k: int) -> np.ndarray:
    """``hlaPredMerge``'s weight checks and normalisation (``R/HIBAG.R:867-880``), float64 on the host."""
    if weight is None:
        return np.full(k, 1.0 / k)
    w = np.asarray(weight, np.float64)
    if w.shape != (k,):
        raise ValueError("Invalid 'weight'.")
    if np.isnan(w).any():
        raise ValueError("'weight' should not have NA/NaN.")
    if (w < 0).any():
        raise ValueError("'weight' should not have a negative value.")
    return w / w.sum()


class _DevicePlan:
    """The library's handle of a :class:`MergePlan` (``hibag_hip_merge_plan_new``)."""

    def __init__(self, plan: MergePlan, device: int):
        k = len(plan.row_of_cell)
        maps = [np.ascontiguousarray(r, np.int32) for r in plan.row_of_cell]
        n_cell = np.array([len(r) for r in maps], np.int32)
        ptrs = (C.c_void_p * k)(*[r.ctypes.data for r in maps])
        h = _lib.lib().hibag_hip_merge_plan_new(k, _as_ptr(n_cell), ptrs, len(plan.hla_allele), int(device))
        if not h:
            raise _lib.HibagHipError(-1, _lib.lib().hibag_hip_last_error().decode())
        self._h = C.c_void_p(h)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            _lib.lib().hibag_hip_merge_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr_array(arrays: Sequence[Optional[np.ndarray]]):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def hlaPredictMerge(models: Sequence[HlaAttrBagClass], snp: Union[HlaSNPGeno, HlaBEDGeno, np.ndarray], weight=None,
                    equivalence: Optional[Dict[str, str]] = None, use_matching: bool = True, ret_dosage: bool = True,
                    ret_postprob: bool = False, max_resolution: str = "", rm_suffix: bool = False, vote: str = "prob",
                    allele_check: bool = True, match_type: str = "Position", same_strand: bool = False,
                    verbose: bool = True) -> HlaAlleleClass:
    """Predict ``snp`` with every model of ``models`` (``HlaAttrBagClass`` of one locus on one device) and merge the
    posteriors as ``hlaPredMerge`` does; the remaining arguments mean what they mean in ``hlaPredict`` and
    ``hlaPredMerge``.  Returns the ``HlaAlleleClass`` the composed call returns, field by field and bit for bit."""
    if isinstance(models, HlaAttrBagClass) or not isinstance(models, (list, tuple)):
        raise TypeError("'models' should be a list of 'hlaAttrBagClass' objects.")
    if not models:
        raise ValueError("No hlaAlleleClass object passed to 'hlaPredMerge()'.")
    for m in models:
        if not isinstance(m, HlaAttrBagClass):
            raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if vote not in _hb._VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    vote_method = _hb._VOTES.index(vote) + 1
    k = len(models)
    locus = models[0].obj.hla_locus
    for m in models:
        if m.obj.hla_locus != locus:
            raise ValueError("The locus should be the same.")
    w = _merge_weights(weight, k)
    hlaAlleleDigit([], max_resolution, rm_suffix)            # (its check of 'max.resolution')
    if k > MAX_MODELS:
        raise ValueError(f"hlaPredictMerge() takes at most {MAX_MODELS} models, not {k}.")
    out = sys.stdout

    # ---- per model: hlaPredict's own front half (R/HIBAG.R:530-715) -- the SNP matching, its verbose text ----
    bed = isinstance(snp, HlaBEDGeno)
    mat = None
    if not bed:
        mat = np.asarray(snp.genotype if isinstance(snp, HlaSNPGeno) else snp)
        if not isinstance(snp, HlaSNPGeno):
            if mat.dtype.kind not in "iufb":
                raise TypeError("is.numeric(snp) is not TRUE")
            if mat.ndim == 1:
                mat = mat.reshape(-1, 1)
        elif mat.ndim != 2:
            raise ValueError("'snp$genotype' must be a matrix [n.snp, n.samp]")
    sels: List[Optional[np.ndarray]] = []
    flips: List[Optional[np.ndarray]] = []
    assembly = None
    sample_id: List = []
    for m in models:
        obj = m.obj
        if verbose:
            s = list(obj.hla_allele)
            if len(s) > 3:
                s = s[:3] + ["..."]
            n_c = len(obj.classifiers)
            print(f"HIBAG model for HLA-{obj.hla_locus}:\n    {n_c} individual classifier{'s' if n_c > 1 else ''}\n"
                  f"    {len(obj.snp_id)} SNPs\n    {obj.n_hla} unique HLA alleles: {', '.join(s)}", file=out)
            print("Prediction:\n    " + ("based on the averaged posterior probabilities" if vote_method == 1
                                          else "by voting from all individual classifiers"), file=out)
        if bed:
            from .snpmatch import plan_snps_for_predict
            p = plan_snps_for_predict(obj, snp, snp.allele_freq, match_type, allele_check, same_strand, verbose, verbose)
            sel, flip, asm = np.asarray(p.sel), p.flip, p.assembly
            sample_id = list(snp.sample_id)
        elif isinstance(snp, HlaSNPGeno):
            from .snpmatch import _row_afreq, plan_snps_for_predict
            p = plan_snps_for_predict(obj, snp, lambda rows: _row_afreq(_as_integer(mat[rows])), match_type, allele_check,
                                      same_strand, verbose, verbose)
            sel, flip, asm = (None if p.identity else np.asarray(p.sel)), p.flip, p.assembly
            sample_id = list(snp.sample_id)
            if len(sample_id) != mat.shape[1]:
                raise ValueError("length(snp$sample.id) == ncol(snp$genotype) is not TRUE")
        else:
            if mat.ndim != 2 or mat.shape[0] != obj.n_snp:
                raise ValueError("length(snp) == object$n.snp is not TRUE" if np.asarray(snp).ndim == 1
                                 else "nrow(snp) == object$n.snp is not TRUE")
            sel, flip, asm = None, None, "auto-silent"
            sample_id = list(range(1, mat.shape[1] + 1))
        if flip is not None and not np.any(flip):
            flip = None
        sels.append(sel)
        flips.append(flip)
        if assembly is None:
            assembly = asm
        if verbose:
            print(f"# of samples: {len(sample_id)}", file=out)
            print(f"Kernel target: {_hb._kernel_info or 'hip'}", file=out)
    n_samp = len(sample_id)

    # ---- the names: hlaPredMerge's (R/HIBAG.R:905-957) ----
    plan = merge_plan([m.obj.hla_allele for m in models], equivalence, max_resolution, rm_suffix)
    if verbose:
        print(f"Aggregate {k} set{'s' if k > 1 else ''} of predictions:")
        for i, (m, r) in enumerate(zip(models, plan.row_of_cell)):
            nh = len({int(x) for x in r[np.cumsum(np.r_[0, np.arange(m.obj.n_hla, 1, -1)])]})     # (its diagonal cells' rows)
            print(f"    {i + 1}. # of unique alleles: {m.obj.n_hla}" + (f" ==>  {nh}" if equivalence else ""))
        print(f"# of unique allele in the merged set = {len(plan.hla_allele)}")

    # ---- the device ----
    device = models[0].device()
    for m in models:
        if m.device() != device:
            raise ValueError(f"hlaPredictMerge(): the models should be on the same device (found devices {device} and {m.device()}); "
                             "replicate a model to the other's device first (HlaAttrBagClass.replicate).")
    # a model listed twice needs a workspace of its own for its second appearance
    used, handles, temps = set(), [], []
    try:
        for m in models:
            if id(m) in used:
                m = m.replicate(device)
                temps.append(m)
            used.add(id(m))
            handles.append(m)
        n_hla, P = len(plan.hla_allele), plan.n_row
        res = dict(h1=np.empty(n_samp, np.int32), h2=np.empty(n_samp, np.int32), prob=np.empty(n_samp, np.float64),
                   matching=np.empty(n_samp, np.float64))
        if ret_dosage:
            res["dosage"] = np.empty((n_hla, n_samp), np.float64)
        if ret_postprob:
            res["postprob"] = np.empty((P, n_samp), np.float64)
        L = _lib.lib()
        dplan = _DevicePlan(plan, device)
        try:
            hs = (C.c_void_p * k)(*[m.handle for m in handles])
            flip32 = [None if f is None else np.ascontiguousarray(np.asarray(f) != 0, np.int32) for f in flips]
            outs = (_as_ptr(res["h1"]), _as_ptr(res["h2"]), _as_ptr(res["prob"]), _as_ptr(res["matching"]),
                    _as_ptr(res.get("dosage")), _as_ptr(res.get("postprob")))
            if bed:
                cols = [np.ascontiguousarray(np.where(s >= 0, snp.bed_index[np.maximum(s, 0)], -1), np.int32) for s in sels]
                _lib.check(L.hibag_hip_predict_merge_bed(dplan.handle, hs, os.fsencode(snp.bed_fn), int(snp.n_bed_samp),
                                                         int(snp.n_bed_snp), _ptr_array(cols), _ptr_array(flip32), vote_method,
                                                         _as_ptr(w), int(bool(use_matching)), *outs))
            else:
                g = _as_integer(mat)
                # the cohort goes up once, whole: where it has many more SNPs than the models use (a genome-wide matrix), only
                # the rows any model uses are handed over (the models' few hundred rows of the cohort)
                if any(s is not None for s in sels):
                    need = np.unique(np.concatenate([np.arange(m.obj.n_snp) if s is None else s[s >= 0]
                                                     for m, s in zip(models, sels)]))
                    if 2 * len(need) < g.shape[0]:
                        pos = np.full(g.shape[0], -1, np.int64)
                        pos[need] = np.arange(len(need))
                        sels = [np.where((np.arange(m.obj.n_snp) if s is None else s) >= 0,
                                         pos[np.maximum(np.arange(m.obj.n_snp) if s is None else s, 0)], -1)
                                for m, s in zip(models, sels)]
                        g = g[need]
                cols = [None if s is None else np.ascontiguousarray(s, np.int32) for s in sels]
                if g.flags.f_contiguous and not g.flags.c_contiguous:
                    gm, snp_major, ld = g.T, 0, 0             # R's memory order: the transpose view is sample-major
                else:
                    gm, snp_major, ld = np.ascontiguousarray(g), 1, n_samp
                _lib.check(L.hibag_hip_predict_merge(dplan.handle, hs, _as_ptr(gm), snp_major, ld, n_samp, int(g.shape[0]),
                                                     _ptr_array(cols), _ptr_array(flip32), vote_method, _as_ptr(w),
                                                     int(bool(use_matching)), *outs))
        finally:
            dplan.close()
    finally:
        for m in temps:
            m.close()

    rv = HlaAlleleClass(locus=locus, sample_id=sample_id, h1=res["h1"], h2=res["h2"], levels=plan.hla_allele,
                        prob=res["prob"], matching=res["matching"], assembly=assembly or "auto")
    if ret_dosage:
        rv.dosage = res["dosage"]
    if ret_postprob:
        rv.postprob = res["postprob"]
        rv.pair_names = plan.pair_names
    return rv
