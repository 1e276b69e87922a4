"""Host-side mirror of the reference's R interface for the prediction path.

Same names, argument meaning and error behaviour as the reference's
``hlaSetKernelTarget`` (``R/HIBAG.R:1668-1674``), ``hlaModelFromObj`` /
``hlaModelToObj`` (``R/HIBAG.R:1135-1178`` / ``:1041-1062``) and ``hlaPredict``
(``R/HIBAG.R:481-818``); the compute goes through the C ABI of
``libhibag_hip.so`` (``include/hibag_hip.h``) and nowhere else.

R is not available on the GPU box, so the thin R layer is restated in Python
(the reference itself has no Python).  PyTorch appears only where a caller
hands over device tensors.
"""

from __future__ import annotations

import ctypes as C
import os
import sys
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import HibagHipError
from .bed import HlaBEDGeno
from .cohort import HlaDeviceCohort
from .model import (NA_INTEGER, Classifier, HlaAttrBagObj, HlaSNPGeno)

_TARGETS_CPU = ("max", "auto.avx2", "base", "sse2", "sse4", "avx", "avx2", "avx512f", "avx512bw",
                "avx512vpopcnt")   # src/LibHLA.cpp:1279-1456, man/hlaSetKernelTarget.Rd
_kernel_target: Optional[str] = None
_kernel_info: str = ""


def hlaSetKernelTarget(cpu: str = "hip") -> List[str]:
    """Select the kernel target.  The reference accepts CPU instruction sets
    (``src/LibHLA.cpp:1266-1475``); this build adds the value ``"hip"`` and
    implements only that: the CPU names raise, as the reference does for a
    target the build does not support (``Rf_error("Not support AVX2.")``)."""
    global _kernel_target, _kernel_info
    cpu = str(cpu)
    if cpu != "hip":
        if cpu in _TARGETS_CPU:
            raise HibagHipError(_lib.lib().hibag_hip_set_kernel_target(cpu.encode(), None, 0),
                                f"Not support {cpu.upper()}: hibag_amd implements the \"hip\" kernel target only.")
        raise ValueError(f"'arg' should be one of \"hip\", {', '.join(repr(t) for t in _TARGETS_CPU)}")
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().hibag_hip_set_kernel_target(b"hip", buf, len(buf)))
    _kernel_target, _kernel_info = "hip", buf.value.decode()
    return [_kernel_info]


def _as_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev_ptr(x):
    """A device address (``tensor.data_ptr()``) or a stream handle, or None, as a C pointer argument."""
    return None if x is None else C.c_void_p(int(x))


def _list_count(v, name: str, limit: int, macro: str) -> int:
    ok = isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not ok and isinstance(v, (float, np.floating)) and float(v).is_integer():
        ok = True
    if not ok or not (1 <= int(v) <= limit):
        raise ValueError(f"'{name}' must be an integer between 1 and {limit} ({macro}): {v!r}")
    return int(v)


def topk_k(k) -> int:
    """The ``k`` of the top-k entries as an int within 1 .. ``HIBAG_HIP_TOPK_MAX``; ``ValueError`` otherwise."""
    return _list_count(k, "k", _lib.TOPK_MAX, "HIBAG_HIP_TOPK_MAX")


def draw_n(n) -> int:
    """The ``n_draw`` of the draw entries as an int within 1 .. ``HIBAG_HIP_DRAW_MAX``; ``ValueError`` otherwise."""
    return _list_count(n, "n", _lib.DRAW_MAX, "HIBAG_HIP_DRAW_MAX")


def _draw_key(seed, sample0) -> tuple:
    """``seed`` (any integer, taken modulo 2^64) and ``sample0`` (>= 0) of the draw entries."""
    for v, what in ((seed, "seed"), (sample0, "sample0")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            raise ValueError(f"'{what}' must be an integer: {v!r}")
    if int(sample0) < 0:
        raise ValueError(f"'sample0' must not be negative: {sample0!r}")
    return int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0)


class HlaAttrBagClass:
    """``hlaAttrBagClass``: an ``hlaAttrBagObj`` plus the native model handle
    (the reference keeps an index into a handle table and frees it from a
    finalizer, ``src/HIBAG.cpp:409-475``)."""

    def __init__(self, obj: HlaAttrBagObj, device: Optional[int] = None,
                 snp_weight: Optional[np.ndarray] = None):
        L = _lib.lib()
        self.obj = obj
        self._h = None
        if device is not None:
            _lib.check(L.hibag_hip_set_device(int(device)))
        h = L.hibag_hip_model_new(int(obj.n_hla), int(obj.n_snp))
        if not h:
            raise HibagHipError(-1, L.hibag_hip_last_error().decode())
        self._h = C.c_void_p(h)
        try:
            for c in obj.classifiers:
                strs = (C.c_char_p * len(c.haplo))(*[s.encode() for s in c.haplo])
                _lib.check(L.hibag_hip_model_add_classifier(
                    self._h, len(c.snpidx), _as_ptr(c.snpidx), len(c.freq), _as_ptr(c.freq), _as_ptr(c.hla), strs))
            if snp_weight is not None:
                sw = np.ascontiguousarray(snp_weight, np.int32)
                if sw.shape != (obj.n_snp,):
                    raise ValueError("snp_weight must have one entry per model SNP")
                _lib.check(L.hibag_hip_model_set_snp_weights(self._h, _as_ptr(sw)))
            _lib.check(L.hibag_hip_model_finalize(self._h))
        except Exception:
            self.close()
            raise

    # attribute access like the R list: model$hla.allele -> model.hla_allele
    def __getattr__(self, name):
        if name in ("obj", "_h"):
            raise AttributeError(name)
        return getattr(self.obj, name)

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise HibagHipError(-4, "the model has been closed")
        return self._h

    def close(self):
        """``hlaClose`` (``R/HIBAG.R:1023-1035``)."""
        for r in self.__dict__.pop("_replicas", {}).values():      # replicas made for hlaPredict(cl=[devices])
            r.close()
        if getattr(self, "_h", None) is not None:
            _lib.lib().hibag_hip_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device(self) -> int:
        """The HIP device the model lives on."""
        return int(_lib.lib().hibag_hip_model_device(self.handle))

    def pair_evals(self) -> int:
        return int(_lib.lib().hibag_hip_model_pair_evals(self.handle))

    def stored_cells(self) -> int:
        """Cell sums per sample that pass 1 stores for pass 2 to read back."""
        return int(_lib.lib().hibag_hip_model_stored_cells(self.handle))

    def second_pass_pairs(self) -> int:
        """Haplotype pairs per sample that pass 2 evaluates again (those of the cells that are not stored)."""
        return int(_lib.lib().hibag_hip_model_second_pass_pairs(self.handle))

    # --- launch status (include/hibag_hip.h "launch status of the device-pointer entries") ---
    def status(self) -> int:
        """0, or the model's sticky fault code (waits for the model's outstanding launches first)."""
        return int(_lib.lib().hibag_hip_model_status(self.handle))

    def clear_status(self):
        _lib.check(_lib.lib().hibag_hip_model_clear_status(self.handle))

    def handover_faults(self) -> int:
        return int(_lib.lib().hibag_hip_model_handover_faults(self.handle))

    def inject_handover_fault(self, which_pass: int):
        """Tests only: the next batch drops the first hand-over of pass 1 or 2."""
        _lib.check(_lib.lib().hibag_hip_test_inject_handover_fault(self.handle, int(which_pass)))

    def set_chunking(self, slots_pass1: int = 0, slots_pass2: int = 0, tail_k: int = 0):
        """Tests only: lower the resident-workgroup figures of pass 1 / pass 2 (never above what the device reported) and
        set the chunks per item of both passes; 0 restores an argument's default (``hibag_hip_test_set_chunking``)."""
        _lib.check(_lib.lib().hibag_hip_test_set_chunking(self.handle, int(slots_pass1), int(slots_pass2), int(tail_k)))

    def last_launch(self) -> dict:
        """Tests only: what the model's most recent passes 1 and 2 launched (``hibag_hip_launch_info`` as a dict)."""
        info = _lib.LaunchInfo()
        _lib.check(_lib.lib().hibag_hip_test_last_launch(self.handle, C.byref(info)))
        return info.as_dict()

    def engine(self, classifier: int):
        """(engine name, K steps) of a classifier as the library finalized it."""
        e, k = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().hibag_hip_model_engine(self.handle, int(classifier), C.byref(e), C.byref(k)))
        return {0: "valu", 1: "fp4", 2: "i8", 3: "i8"}[e.value], k.value

    def replicate(self, device: int) -> "HlaAttrBagClass":
        """A finalized copy of the model on another (or the same) device: ``hibag_hip_model_replicate``."""
        h = _lib.lib().hibag_hip_model_replicate(self.handle, int(device))
        if not h:
            raise HibagHipError(-2, _lib.lib().hibag_hip_last_error().decode())
        r = object.__new__(HlaAttrBagClass)
        r.obj = self.obj
        r._h = C.c_void_p(h)
        return r

    def shard(self, shard: int, n_shards: int, device: int) -> "HlaAttrBagClass":
        """Classifiers ``hibag_hip_shard_bounds(C, n_shards, shard)`` of the model as a model of their own on ``device``,
        with the full model's per-SNP classifier counts: ``hibag_hip_model_shard``."""
        h = _lib.lib().hibag_hip_model_shard(self.handle, int(shard), int(n_shards), int(device))
        if not h:
            raise HibagHipError(-2, _lib.lib().hibag_hip_last_error().decode())
        r = object.__new__(HlaAttrBagClass)
        r.obj = self.obj                      # (alleles, SNPs: the full model's; the shard's classifiers live in the library)
        r._h = C.c_void_p(h)
        return r

    def mutation_table(self) -> np.ndarray:
        t = np.empty(257, np.float64)
        _lib.check(_lib.lib().hibag_hip_model_mutation_table(self.handle, _as_ptr(t)))
        return t

    # --- timing of the kernels (HIP events on the launch stream) ---
    def set_timing(self, enabled=True):
        """True / False: HIP events around every kernel class or none; a sequence of kernel names (``"total"``, ``"accum"``,
        ``"pack"``, ``"finish"``): events around those only (``hibag_hip_set_timing``'s mask form)."""
        if isinstance(enabled, (list, tuple, set, frozenset)):
            ids = {v: k for k, v in _lib.KERNEL_NAMES.items()}
            code = 2 * sum(1 << ids[name] for name in set(enabled))
        else:
            code = int(bool(enabled))
        _lib.check(_lib.lib().hibag_hip_set_timing(self.handle, code))

    def reset_timing(self):
        _lib.check(_lib.lib().hibag_hip_reset_timing(self.handle))

    def get_timing(self) -> dict:
        out = {}
        for k, name in _lib.KERNEL_NAMES.items():
            ms, n = C.c_double(0), C.c_int64(0)
            _lib.check(_lib.lib().hibag_hip_get_timing(self.handle, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    # --- raw entry points -------------------------------------------------
    # Every host-pointer entry of the C ABI is `hibag_hip_predict[_topk|_draw]<route>(model, <route's arguments>, vote_method,
    # <family's own arguments>, <outputs>)`.  A route (`_route_*`) validates and marshals its arguments once, for all three
    # families: it returns (the entry's suffix, the C arguments in front of vote_method, n_samp).  A tail (`_six`, `_list`)
    # says which family is called: (the entry's stem, its own C arguments, the keys of its outputs in C order, n -> arrays).
    def _genomat(self, genomat) -> np.ndarray:
        g = np.ascontiguousarray(genomat, np.int32)
        if g.ndim != 2 or g.shape[1] != self.obj.n_snp:
            raise ValueError("genomat must be [n_samp, n.snp] int32")
        return g

    def _model_col_flip(self, snp_col, flip):
        col = np.ascontiguousarray(snp_col, np.int32)
        if col.shape != (self.obj.n_snp,):
            raise ValueError("snp_col must have one entry per model SNP")
        return col, (None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, np.int32))

    def _route_raw(self, genomat):
        g = self._genomat(genomat)
        return "", (_as_ptr(g), g.shape[0]), g.shape[0]

    def _route_mapped(self, genomat, snp_col, flip):
        g = np.ascontiguousarray(genomat, np.int32)
        if g.ndim != 2:
            raise ValueError("genomat must be [n_samp, n_geno_snp]")
        col, fl = self._model_col_flip(snp_col, flip)
        return "_mapped", (_as_ptr(g), g.shape[0], g.shape[1], _as_ptr(col), _as_ptr(fl)), g.shape[0]

    def _route_snp_major(self, genomat, snp_col, flip):
        g = np.asarray(genomat)
        if g.ndim != 2 or g.dtype != np.int32 or g.strides[1] != 4 or g.strides[0] % 4 or (g.shape[0] > 1 and g.strides[0] < 4 * g.shape[1]):
            g = np.ascontiguousarray(g, np.int32)
            if g.ndim != 2:
                raise ValueError("genomat must be [n_geno_snp, n_samp]")
        col = None
        if snp_col is not None:
            col, _ = self._model_col_flip(snp_col, None)
        elif g.shape[0] < self.obj.n_snp:
            raise ValueError("nrow(snp) == object$n.snp is not TRUE")
        fl = None if flip is None else np.ascontiguousarray(np.asarray(flip) != 0, np.int32)
        n = g.shape[1]
        ld = g.strides[0] // 4 if g.shape[0] > 1 else max(n, 1)
        return "_snp_major", (_as_ptr(g), ld, n, max(g.shape[0], 1), _as_ptr(col), _as_ptr(fl)), n

    def _route_bed(self, bed_fn, n_samp, n_snp, snp_col, flip):
        col, fl = self._model_col_flip(snp_col, flip)
        return "_bed", (os.fsencode(bed_fn), int(n_samp), int(n_snp), _as_ptr(col), _as_ptr(fl)), int(n_samp)

    def _route_cohort(self, cohort, snp_col, flip, first, count):
        h = cohort.handle
        col, fl = self._model_col_flip(snp_col, flip)
        first = int(first)
        n = cohort.n_samp - first if count is None else int(count)
        return "_cohort", (h, first, n, _as_ptr(col), _as_ptr(fl)), n

    def _outputs(self, n: int, want_dosage: bool, want_prob: bool) -> dict:
        """The output arrays of ``PredictHLA`` for n samples (every element is written by the library)."""
        out = dict(h1=np.empty(n, np.int32), h2=np.empty(n, np.int32), prob=np.empty(n, np.float64), matching=np.empty(n, np.float64))
        if want_dosage:
            out["dosage"] = np.empty((n, self.obj.n_hla), np.float64)
        if want_prob:
            out["postprob"] = np.empty((n, self.obj.n_cell), np.float64)
        return out

    def _six(self, want_dosage: bool, want_prob: bool):
        return ("hibag_hip_predict", (), ("h1", "h2", "prob", "matching", "dosage", "postprob"),
                lambda n: self._outputs(n, want_dosage, want_prob))

    @staticmethod
    def _list(family: str, extra: tuple):
        """The list entries' tail: ``family`` "topk" with ``extra`` (k,), or "draw" with (n_draw, seed, sample0)."""
        k = extra[0]
        return ("hibag_hip_predict_" + family, extra, ("h1", "h2", "prob", "matching"),
                lambda n: dict(h1=np.empty((n, k), np.int32), h2=np.empty((n, k), np.int32), prob=np.empty((n, k), np.float64),
                               matching=np.empty(n, np.float64)))

    def _call(self, route, vote_method: int, tail) -> dict:
        suffix, head, n = route
        stem, extra, keys, make = tail
        out = make(max(n, 0))
        _lib.check(getattr(_lib.lib(), stem + suffix)(self.handle, *head, int(vote_method), *extra,
                                                      *[_as_ptr(out.get(k)) for k in keys]))
        return out

    def predict_raw(self, genomat: np.ndarray, vote_method: int = 1, want_dosage: bool = True,
                    want_prob: bool = False) -> dict:
        """``CAttrBag_Model::PredictHLA`` on host arrays: ``genomat`` int32 [n_samp, n_snp]."""
        return self._call(self._route_raw(genomat), vote_method, self._six(want_dosage, want_prob))

    def predict_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray] = None,
                       vote_method: int = 1, want_dosage: bool = True, want_prob: bool = False) -> dict:
        """``PredictHLA`` on the COHORT's own matrix ``genomat`` [n_samp, n_geno_snp] (``hibag_hip_predict_mapped``):
        ``snp_col[k]`` = column of model SNP k (-1 = absent), ``flip[k]`` = reverse its allele count; the
        selection and the flip happen on the device while the genotypes are packed."""
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, self._six(want_dosage, want_prob))

    def predict_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray] = None, flip: Optional[np.ndarray] = None,
                          vote_method: int = 1, want_dosage: bool = True, want_prob: bool = False) -> dict:
        """``PredictHLA`` on a SNP-MAJOR matrix ``genomat`` [n_geno_snp, n_samp] in C order -- numpy's own layout for the
        [SNP, sample] matrix of an ``hlaSNPGenoClass`` (``hibag_hip_predict_snp_major``): row ``snp_col[k]`` holds model SNP k
        (-1 = absent; ``None`` = row k), ``flip[k]`` reverses its allele count.  Nothing is transposed on the host."""
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, self._six(want_dosage, want_prob))

    def predict_bed(self, bed_fn: str, n_samp: int, n_snp: int, snp_col: np.ndarray, flip: Optional[np.ndarray] = None,
                    vote_method: int = 1, want_dosage: bool = True, want_prob: bool = False) -> dict:
        """``PredictHLA`` on every sample of a PLINK BED file (``hibag_hip_predict_bed``):
        ``snp_col[k]`` = 0-based .bim index of model SNP k (-1 = absent), ``flip[k]`` =
        reverse the allele count of SNP k."""
        return self._call(self._route_bed(bed_fn, n_samp, n_snp, snp_col, flip), vote_method, self._six(want_dosage, want_prob))

    def predict_cohort(self, cohort, snp_col: np.ndarray, flip: Optional[np.ndarray] = None, vote_method: int = 1,
                       want_dosage: bool = True, want_prob: bool = False, first: int = 0, count: Optional[int] = None) -> dict:
        """``PredictHLA`` on samples ``[first, first + count)`` of a resident cohort (``hibag_hip_predict_cohort``;
        ``cohort``: an ``HlaDeviceCohort``): ``snp_col[k]`` = resident row of model SNP k (-1 = absent), ``flip[k]`` =
        reverse its allele count.  Nothing but the row map goes up."""
        return self._call(self._route_cohort(cohort, snp_col, flip, first, count), vote_method, self._six(want_dosage, want_prob))

    def predict_oob(self, genomat: np.ndarray, samp_num) -> dict:
        """``hlaOutOfBag``'s per-classifier predictions (``R/HIBAG.R:1320-1334``) in one batched call
        (``hibag_hip_predict_oob``): classifier c, as a one-classifier model of its own, predicts every sample s with
        ``samp_num[c, s] == 0``.  ``genomat`` int32 [n_samp, n_snp] holds the model's training samples in
        ``sample_id`` order, ``samp_num`` [n_classifier, n_samp] their bootstrap counts.  Returns ``h1``, ``h2``
        (0-based, NA = INT_MIN where not predicted) and ``prob`` (0 there), each [n_classifier, n_samp]."""
        g = self._genomat(genomat)
        n, nc = g.shape[0], len(self.obj.classifiers)
        sn = np.ascontiguousarray(samp_num, np.int32)
        if sn.shape != (nc, n):
            raise ValueError(f"samp_num must be [n_classifier, n_samp] = [{nc}, {n}]")
        out = {"h1": np.empty((nc, n), np.int32), "h2": np.empty((nc, n), np.int32), "prob": np.empty((nc, n), np.float64)}
        _lib.check(_lib.lib().hibag_hip_predict_oob(self.handle, _as_ptr(g), n, _as_ptr(sn), _as_ptr(out["h1"]),
                                                    _as_ptr(out["h2"]), _as_ptr(out["prob"])))
        return out

    def knock_variants(self) -> int:
        """The model's (classifier, SNP of that classifier) pairs: the rows of :meth:`predict_oob_knock` ahead of the base
        rows (``hibag_hip_oob_knock_variants``)."""
        n = C.c_int(0)
        _lib.check(_lib.lib().hibag_hip_oob_knock_variants(self.handle, C.byref(n)))
        return n.value

    def predict_oob_knock(self, genomat: np.ndarray, samp_num, truth=None, call_threshold: float = float("nan"),
                          raw: bool = False) -> dict:
        """The out-of-bag SNP knock-out in one device call (``hibag_hip_oob_knock``): row ``v = snp_off[c] + j`` is
        classifier c, as a one-classifier model of its own, predicting its out-of-bag samples with its j-th SNP set to
        missing; rows ``n_variant + c`` are the base rows, nothing knocked out (:meth:`predict_oob`'s row c).
        ``genomat`` and ``samp_num`` as for :meth:`predict_oob`; ``truth`` int32 [n_samp, 2], the true alleles as 0-based
        indices of the model's alleles, NA = INT_MIN for a sample that is not counted (``None``: nobody is).  Returns
        ``tally`` int64 [n_variant + n_classifier, 5] -- ``n_ind``, ``n_call``, ``crt_ind``, ``crt_haplo``, ``n_changed`` as
        ``hlaCompareAllele`` counts them --, ``classifier`` and ``snp`` (the model SNP index) of every variant row, and with
        ``raw=True`` the predictions ``h1``, ``h2``, ``prob`` [n_variant + n_classifier, n_samp] (NA / 0 in the bag)."""
        g = self._genomat(genomat)
        n, nc = g.shape[0], len(self.obj.classifiers)
        sn = np.ascontiguousarray(samp_num, np.int32)
        if sn.shape != (nc, n):
            raise ValueError(f"samp_num must be [n_classifier, n_samp] = [{nc}, {n}]")
        if truth is None:
            tr = np.full((n, 2), np.iinfo(np.int32).min, np.int32)
        else:
            tr = np.asarray(truth)
            if tr.dtype.kind not in "iu":
                raise TypeError("truth must be an integer array")
            if tr.shape != (n, 2):
                raise ValueError(f"truth must be [n_samp, 2] = [{n}, 2]")
            tr = np.ascontiguousarray(tr, np.int32)
            if np.any((tr != np.iinfo(np.int32).min) & ((tr < 0) | (tr >= self.obj.n_hla))):
                raise ValueError("truth holds an index outside the model's alleles")
        nv = self.knock_variants()
        rows = nv + nc
        out = {"tally": np.empty((rows, 5), np.int64), "n_variant": nv,
               "classifier": np.repeat(np.arange(nc, dtype=np.int32), [len(c.snpidx) for c in self.obj.classifiers]),
               "snp": np.concatenate([np.asarray(c.snpidx, np.int32) for c in self.obj.classifiers] + [np.empty(0, np.int32)])}
        if raw:
            out.update(h1=np.empty((rows, n), np.int32), h2=np.empty((rows, n), np.int32), prob=np.empty((rows, n), np.float64))
        _lib.check(_lib.lib().hibag_hip_oob_knock(self.handle, _as_ptr(g), n, _as_ptr(sn), _as_ptr(tr), float(call_threshold),
                                                  _as_ptr(out["tally"]), _as_ptr(out.get("h1")), _as_ptr(out.get("h2")),
                                                  _as_ptr(out.get("prob"))))
        return out

    def predict_masked(self, geno: np.ndarray, use, vote_method: int = 1, want_dosage: bool = True,
                       want_prob: bool = False) -> dict:
        """``hibag_hip_predict_masked``: a per-sample classifier mask.  Sample s gets what ``predict_raw`` returns for it
        from the model of the classifiers c with ``use[c, s] != 0`` (in model order, with that sub-model's own SNP weights),
        bit for bit; a sample no classifier is used for gets call NA, ``prob`` 0, ``matching`` NaN.  ``geno`` int32
        [n_samp, n_snp], ``use`` [n_classifier, n_samp] (bool or integer; nonzero = takes part).  Returns a dict like
        :meth:`predict_raw`'s."""
        g = self._genomat(geno)
        n, nc = g.shape[0], len(self.obj.classifiers)
        u = np.asarray(use)
        if u.dtype.kind not in "biu":
            raise TypeError("use must be a boolean or integer array")
        if u.shape != (nc, n):
            raise ValueError(f"use must be [n_classifier, n_samp] = [{nc}, {n}]")
        if int(vote_method) not in (1, 2):
            raise ValueError("Invalid 'vote_method'.")
        u = np.ascontiguousarray(u != 0, np.uint8)
        return self._call(("_masked", (_as_ptr(g), n, _as_ptr(u)), n), vote_method, self._six(want_dosage, want_prob))

    def predict_prefix(self, genomat: np.ndarray, sizes) -> dict:
        """``hibag_hip_predict_prefix``: for every ``sizes[i]`` (strictly ascending, 1 .. n_classifier) what
        ``predict_raw`` (vote by probability) returns for the model of the first ``sizes[i]`` classifiers
        (``hlaSubModelObj``) -- ``h1``, ``h2``, ``prob``, ``matching``, each [n_sizes, n_samp] -- from one pass 1.
        ``genomat`` int32 [n_samp, n_snp]."""
        g = self._genomat(genomat)
        sz = np.ascontiguousarray(sizes, np.int32)
        if sz.ndim != 1:
            raise ValueError("sizes must be a vector")
        n, k = g.shape[0], len(sz)
        out = {"h1": np.empty((k, n), np.int32), "h2": np.empty((k, n), np.int32), "prob": np.empty((k, n), np.float64),
               "matching": np.empty((k, n), np.float64)}
        _lib.check(_lib.lib().hibag_hip_predict_prefix(self.handle, _as_ptr(g), n, _as_ptr(sz), k, _as_ptr(out["h1"]),
                                                       _as_ptr(out["h2"]), _as_ptr(out["prob"]), _as_ptr(out["matching"])))
        return out

    def prefix_accum_ms(self) -> float:
        """Event time (ms) of ``k_prefix_accum`` in the model's last ``predict_prefix`` call."""
        ms = C.c_double()
        _lib.check(_lib.lib().hibag_hip_predict_prefix_ms(self.handle, C.byref(ms)))
        return ms.value

    # --- the list entries: the k best pairs of every sample (hibag_hip_predict_topk and its routes; include/hibag_hip.h
    # "top-k") and pairs drawn from its posterior (hibag_hip_predict_draw and its routes; "posterior draws"): the routes
    # above with the list tail.
    def predict_topk(self, genomat: np.ndarray, k: int, vote_method: int = 1) -> dict:
        """``hibag_hip_predict_topk``: per sample the ``k`` largest cells of the normalised posterior matrix (what
        ``predict_raw(..., want_prob=True)`` returns as ``postprob``) selected on the device -- ``h1``, ``h2`` (0-based,
        NA = INT_MIN in the ranks no pair qualifies for) and ``prob`` (0 there), each [n_samp, k], descending, equal values
        in pair order, and ``matching`` [n_samp].  Rank 0 is ``predict_raw``'s call.  ``genomat`` int32 [n_samp, n_snp]."""
        tail = self._list("topk", (topk_k(k),))
        return self._call(self._route_raw(genomat), vote_method, tail)

    def predict_topk_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray], k: int,
                            vote_method: int = 1) -> dict:
        """:meth:`predict_topk` on the cohort's own matrix [n_samp, n_geno_snp], as :meth:`predict_mapped`."""
        tail = self._list("topk", (topk_k(k),))
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, tail)

    def predict_topk_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray], flip: Optional[np.ndarray], k: int,
                               vote_method: int = 1) -> dict:
        """:meth:`predict_topk` on a SNP-major matrix [n_geno_snp, n_samp] in C order, as :meth:`predict_snp_major`."""
        tail = self._list("topk", (topk_k(k),))
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, tail)

    def predict_topk_bed(self, bed_fn: str, n_samp: int, n_snp: int, snp_col: np.ndarray, flip: Optional[np.ndarray], k: int,
                         vote_method: int = 1) -> dict:
        """:meth:`predict_topk` on every sample of a PLINK BED file, as :meth:`predict_bed`."""
        tail = self._list("topk", (topk_k(k),))
        return self._call(self._route_bed(bed_fn, n_samp, n_snp, snp_col, flip), vote_method, tail)

    def predict_topk_cohort(self, cohort, snp_col: np.ndarray, flip: Optional[np.ndarray], k: int, vote_method: int = 1,
                            first: int = 0, count: Optional[int] = None) -> dict:
        """:meth:`predict_topk` on samples ``[first, first + count)`` of a resident cohort, as :meth:`predict_cohort`."""
        tail = self._list("topk", (topk_k(k),))
        return self._call(self._route_cohort(cohort, snp_col, flip, first, count), vote_method, tail)

    def predict_topk_device(self, d_geno, n_samp: int, k: int, d_h1, d_h2, d_prob, d_matching=None, vote_method: int = 1,
                            stream=None):
        """Device-pointer form of :meth:`predict_topk`; arguments are ints (``tensor.data_ptr()``) or None."""
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_topk_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), int(k), p(d_h1), p(d_h2), p(d_prob), p(d_matching), p(stream)))

    def predict_draw(self, genomat: np.ndarray, n: int, seed: int, vote_method: int = 1, sample0: int = 0) -> dict:
        """``hibag_hip_predict_draw``: per sample ``n`` allele pairs drawn on the device from the normalised posterior
        matrix (what ``predict_raw(..., want_prob=True)`` returns as ``postprob``) -- ``h1``, ``h2`` (0-based, NA = INT_MIN
        for a sample without a positive cell) and ``prob`` (the drawn pair's posterior), each [n_samp, n], and
        ``matching`` [n_samp].  Draw t of sample s is a function of (``seed``, ``sample0 + s``, t) and the sample's posterior
        alone.  ``genomat`` int32 [n_samp, n_snp]."""
        tail = self._list("draw", (draw_n(n),) + _draw_key(seed, sample0))
        return self._call(self._route_raw(genomat), vote_method, tail)

    def predict_draw_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray], n: int, seed: int,
                            vote_method: int = 1, sample0: int = 0) -> dict:
        """:meth:`predict_draw` on the cohort's own matrix [n_samp, n_geno_snp], as :meth:`predict_mapped`."""
        tail = self._list("draw", (draw_n(n),) + _draw_key(seed, sample0))
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, tail)

    def predict_draw_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray], flip: Optional[np.ndarray], n: int,
                               seed: int, vote_method: int = 1, sample0: int = 0) -> dict:
        """:meth:`predict_draw` on a SNP-major matrix [n_geno_snp, n_samp] in C order, as :meth:`predict_snp_major`."""
        tail = self._list("draw", (draw_n(n),) + _draw_key(seed, sample0))
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, tail)

    def predict_draw_bed(self, bed_fn: str, n_samp: int, n_snp: int, snp_col: np.ndarray, flip: Optional[np.ndarray], n: int,
                         seed: int, vote_method: int = 1, sample0: int = 0) -> dict:
        """:meth:`predict_draw` on every sample of a PLINK BED file, as :meth:`predict_bed`."""
        tail = self._list("draw", (draw_n(n),) + _draw_key(seed, sample0))
        return self._call(self._route_bed(bed_fn, n_samp, n_snp, snp_col, flip), vote_method, tail)

    def predict_draw_cohort(self, cohort, snp_col: np.ndarray, flip: Optional[np.ndarray], n: int, seed: int,
                            vote_method: int = 1, first: int = 0, count: Optional[int] = None, sample0: int = 0) -> dict:
        """:meth:`predict_draw` on samples ``[first, first + count)`` of a resident cohort, as :meth:`predict_cohort`.
        ``sample0`` is the caller's index of sample ``first`` (``first`` is not added to it): ``sample0=first`` draws what
        a call over the whole cohort draws for these samples."""
        tail = self._list("draw", (draw_n(n),) + _draw_key(seed, sample0))
        return self._call(self._route_cohort(cohort, snp_col, flip, first, count), vote_method, tail)

    def predict_draw_device(self, d_geno, n_samp: int, n: int, seed: int, d_h1, d_h2, d_prob, d_matching=None,
                            vote_method: int = 1, sample0: int = 0, stream=None):
        """Device-pointer form of :meth:`predict_draw`; pointer arguments are ints (``tensor.data_ptr()``) or None."""
        p = _dev_ptr
        seed, sample0 = _draw_key(seed, sample0)
        _lib.check(_lib.lib().hibag_hip_predict_draw_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), int(n), seed, sample0, p(d_h1), p(d_h2), p(d_prob),
            p(d_matching), p(stream)))

    # --- the group entries: per sample and partition of the alleles the best pair of groups under the collapsed posterior
    # (hibag_hip_predict_groups and its routes; include/hibag_hip.h "allele groups"): the routes above with the group tail.
    def groups_plan(self, groups) -> "GroupsPlan":
        """The device plan of ``groups`` -- an ``HlaAlleleGroups`` (``hibag_amd.groups``) or an integer matrix
        [n_part, n_hla] of group ids -- for this model (``hibag_hip_groups_create``).  Made once, used by any number of
        ``predict_groups*`` calls of this model; ``close()`` frees it."""
        return GroupsPlan(self, getattr(groups, "group_of", groups))

    def _groups(self, plan, want_dosage: bool):
        if not isinstance(plan, GroupsPlan):
            raise TypeError("plan must come from HlaAttrBagClass.groups_plan()")
        q, d = plan.n_part, plan.n_level
        return ("hibag_hip_predict_groups", (plan.handle,), ("g1", "g2", "prob", "matching", "dosage"),
                lambda n: dict(g1=np.empty((n, q), np.int32), g2=np.empty((n, q), np.int32), prob=np.empty((n, q), np.float64),
                               matching=np.empty(n, np.float64), **({"dosage": np.empty((n, d), np.float64)} if want_dosage else {})))

    def predict_groups(self, genomat: np.ndarray, plan, vote_method: int = 1, want_dosage: bool = True) -> dict:
        """``hibag_hip_predict_groups``: per sample and partition of ``plan`` the best pair of groups under the posterior
        collapsed over the groups -- ``g1``, ``g2`` (group indices, g1 <= g2, NA = INT_MIN where no pair qualifies) and
        ``prob``, each [n_samp, n_part] --, ``matching`` [n_samp] and, with ``want_dosage``, the expected dosage of every
        group ``dosage`` [n_samp, n_level] (partition q's groups from ``plan.offsets[q]``).  With the identity partition these
        are ``predict_raw``'s ``h1``, ``h2``, ``prob`` and ``dosage`` bit for bit.  ``genomat`` int32
        [n_samp, n_snp]."""
        return self._call(self._route_raw(genomat), vote_method, self._groups(plan, want_dosage))

    def predict_groups_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray], plan,
                              vote_method: int = 1, want_dosage: bool = True) -> dict:
        """:meth:`predict_groups` on the cohort's own matrix [n_samp, n_geno_snp], as :meth:`predict_mapped`."""
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, self._groups(plan, want_dosage))

    def predict_groups_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray], flip: Optional[np.ndarray], plan,
                                 vote_method: int = 1, want_dosage: bool = True) -> dict:
        """:meth:`predict_groups` on a SNP-major matrix [n_geno_snp, n_samp] in C order, as :meth:`predict_snp_major`."""
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, self._groups(plan, want_dosage))

    def predict_groups_bed(self, bed_fn: str, n_samp: int, n_snp: int, snp_col: np.ndarray, flip: Optional[np.ndarray], plan,
                           vote_method: int = 1, want_dosage: bool = True) -> dict:
        """:meth:`predict_groups` on every sample of a PLINK BED file, as :meth:`predict_bed`."""
        return self._call(self._route_bed(bed_fn, n_samp, n_snp, snp_col, flip), vote_method, self._groups(plan, want_dosage))

    def predict_groups_cohort(self, cohort, snp_col: np.ndarray, flip: Optional[np.ndarray], plan, vote_method: int = 1,
                              want_dosage: bool = True, first: int = 0, count: Optional[int] = None) -> dict:
        """:meth:`predict_groups` on samples ``[first, first + count)`` of a resident cohort, as :meth:`predict_cohort`."""
        return self._call(self._route_cohort(cohort, snp_col, flip, first, count), vote_method, self._groups(plan, want_dosage))

    def predict_groups_device(self, d_geno, n_samp: int, plan, d_g1, d_g2, d_prob, d_matching=None, d_dosage=None,
                              vote_method: int = 1, stream=None):
        """Device-pointer form of :meth:`predict_groups`; pointer arguments are ints (``tensor.data_ptr()``) or None."""
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_groups_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), plan.handle, p(d_g1), p(d_g2), p(d_prob), p(d_matching),
            p(d_dosage), p(stream)))

    # --- the given entries: per sample the best allele pair among the cells consistent with two allele sets, a per-sample
    # INPUT (hibag_hip_predict_given and its routes; include/hibag_hip.h "partial typing"): the routes above with the given tail.
    def given_words(self) -> int:
        """W: the uint32 words of one allele set of this model, (n_hla + 31) // 32."""
        return (int(self.obj.n_hla) + 31) // 32

    def _given(self, allow, want_dosage: bool):
        a = getattr(allow, "pack", None)
        a = np.asarray(a() if callable(a) else allow)
        if a.dtype != np.uint32 or a.ndim != 3 or a.shape[1:] != (2, self.given_words()):
            raise ValueError(f"allow must be a uint32 array [n_samp, 2, W = {self.given_words()}] (HlaAlleleConstraint.pack()), "
                             f"got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        nh = int(self.obj.n_hla)

        def make(n):
            if a.shape[0] != n:
                raise ValueError(f"allow holds {a.shape[0]} samples, the genotypes {n}")
            return dict(h1=np.empty(n, np.int32), h2=np.empty(n, np.int32), prob=np.empty(n, np.float64),
                        support=np.empty(n, np.float64), matching=np.empty(n, np.float64),
                        **({"dosage": np.empty((n, nh), np.float64)} if want_dosage else {}))
        return ("hibag_hip_predict_given", (_as_ptr(a),), ("h1", "h2", "prob", "support", "matching", "dosage"), make)

    def predict_given(self, genomat: np.ndarray, allow, vote_method: int = 1, want_dosage: bool = False) -> dict:
        """``hibag_hip_predict_given``: per sample the best allele pair among the cells CONSISTENT with the sample's two
        allele sets -- ``h1``, ``h2`` (0-based, h1 <= h2, NA = INT_MIN where no consistent cell qualifies), ``prob`` (that
        cell's JOINT posterior), ``support`` (the consistent cells' posterior mass, added in pair order), ``matching``, each
        [n_samp], and with ``want_dosage`` the allele ``dosage`` [n_samp, n_hla] restricted to the consistent cells (joint
        too).  ``allow``: uint32 [n_samp, 2, W] (allele h = bit h % 32 of word h // 32 of set A (0) or B (1)), or an
        ``HlaAlleleConstraint``.  With both sets full these are ``predict_raw``'s ``h1``, ``h2``, ``prob`` and ``dosage`` bit
        for bit.  ``genomat`` int32 [n_samp, n_snp]."""
        return self._call(self._route_raw(genomat), vote_method, self._given(allow, want_dosage))

    def predict_given_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray], allow,
                             vote_method: int = 1, want_dosage: bool = False) -> dict:
        """:meth:`predict_given` on the cohort's own matrix [n_samp, n_geno_snp], as :meth:`predict_mapped`."""
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, self._given(allow, want_dosage))

    def predict_given_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray], flip: Optional[np.ndarray], allow,
                                vote_method: int = 1, want_dosage: bool = False) -> dict:
        """:meth:`predict_given` on a SNP-major matrix [n_geno_snp, n_samp] in C order, as :meth:`predict_snp_major`."""
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, self._given(allow, want_dosage))

    def predict_given_bed(self, bed_fn: str, n_samp: int, n_snp: int, snp_col: np.ndarray, flip: Optional[np.ndarray], allow,
                          vote_method: int = 1, want_dosage: bool = False) -> dict:
        """:meth:`predict_given` on every sample of a PLINK BED file, as :meth:`predict_bed`."""
        return self._call(self._route_bed(bed_fn, n_samp, n_snp, snp_col, flip), vote_method, self._given(allow, want_dosage))

    def predict_given_cohort(self, cohort, snp_col: np.ndarray, flip: Optional[np.ndarray], allow, vote_method: int = 1,
                             want_dosage: bool = False, first: int = 0, count: Optional[int] = None) -> dict:
        """:meth:`predict_given` on samples ``[first, first + count)`` of a resident cohort, as :meth:`predict_cohort`;
        row i of ``allow`` belongs to sample ``first + i``."""
        return self._call(self._route_cohort(cohort, snp_col, flip, first, count), vote_method, self._given(allow, want_dosage))

    def predict_given_device(self, d_geno, n_samp: int, d_allow, d_h1, d_h2, d_prob, d_support, d_matching=None, d_dosage=None,
                             vote_method: int = 1, stream=None):
        """Device-pointer form of :meth:`predict_given`; pointer arguments are ints (``tensor.data_ptr()``) or None."""
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_given_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), p(d_allow), p(d_h1), p(d_h2), p(d_prob), p(d_support),
            p(d_matching), p(d_dosage), p(stream)))

    # --- the family entries: per sample the best allele pair under its posterior weighted by its parents' results
    # (hibag_hip_predict_family and its routes; include/hibag_hip.h "pedigrees"): the routes above with the family tail.
    def _family_args(self, pedigree, prior, n: Optional[int] = None):
        ped = np.asarray(pedigree)
        if ped.dtype.kind not in "iu" or ped.ndim != 2 or ped.shape[1] != 2:
            raise ValueError(f"pedigree must be an integer array [n_samp, 2] of (father, mother) sample indices, got {ped.dtype} {ped.shape}")
        if n is not None and ped.shape[0] != n:
            raise ValueError(f"pedigree holds {ped.shape[0]} samples, the genotypes {n}")
        ped = np.ascontiguousarray(ped, np.int32)
        pr = None
        if prior is not None:
            pr = np.ascontiguousarray(prior, np.float64)
            if pr.shape != (int(self.obj.n_hla),):
                raise ValueError(f"prior must hold one entry per allele of the model ({int(self.obj.n_hla)}), got {pr.shape}")
        return ped, pr

    def _family(self, pedigree, prior, want_dosage: bool):
        ped, pr = self._family_args(pedigree, prior)
        nh = int(self.obj.n_hla)

        def make(n):
            if ped.shape[0] != n:
                raise ValueError(f"pedigree holds {ped.shape[0]} samples, the genotypes {n}")
            return dict(h1=np.empty(n, np.int32), h2=np.empty(n, np.int32), prob=np.empty(n, np.float64),
                        support=np.empty(n, np.float64), matching=np.empty(n, np.float64),
                        **({"dosage": np.empty((n, nh), np.float64)} if want_dosage else {}))
        return ("hibag_hip_predict_family", (_as_ptr(ped), _as_ptr(pr)), ("h1", "h2", "prob", "support", "matching", "dosage"), make)

    def predict_family(self, genomat: np.ndarray, pedigree, prior=None, vote_method: int = 1, want_dosage: bool = False) -> dict:
        """``hibag_hip_predict_family``: per sample the best allele pair under its own posterior WEIGHTED by the Mendelian
        transmission probability its parents' results give each pair -- ``h1``, ``h2`` (0-based, h1 <= h2, NA = INT_MIN
        where no pair qualifies), ``prob`` (that pair's JOINT weighted posterior), ``support`` (the weighted mass of all
        pairs, added in pair order), ``matching``, each [n_samp], and with ``want_dosage`` the weighted allele ``dosage``
        [n_samp, n_hla] (joint too).  ``pedigree``: int [n_samp, 2], (father, mother) as sample indices of this call, -1 for
        "not in this call"; parents must precede their children.  ``prior``: float [n_hla], finite and > 0, or None (all
        1.0).  For a sample without known parents these are ``predict_raw``'s ``h1``, ``h2``, ``prob`` and ``dosage`` bit for
        bit.  ``genomat`` int32 [n_samp, n_snp]."""
        return self._call(self._route_raw(genomat), vote_method, self._family(pedigree, prior, want_dosage))

    def predict_family_mapped(self, genomat: np.ndarray, snp_col: np.ndarray, flip: Optional[np.ndarray], pedigree, prior=None,
                              vote_method: int = 1, want_dosage: bool = False) -> dict:
        """:meth:`predict_family` on the cohort's own matrix [n_samp, n_geno_snp], as :meth:`predict_mapped`."""
        return self._call(self._route_mapped(genomat, snp_col, flip), vote_method, self._family(pedigree, prior, want_dosage))

    def predict_family_snp_major(self, genomat: np.ndarray, snp_col: Optional[np.ndarray], flip: Optional[np.ndarray], pedigree,
                                 prior=None, vote_method: int = 1, want_dosage: bool = False) -> dict:
        """:meth:`predict_family` on a SNP-major matrix [n_geno_snp, n_samp] in C order, as :meth:`predict_snp_major`."""
        return self._call(self._route_snp_major(genomat, snp_col, flip), vote_method, self._family(pedigree, prior, want_dosage))

    def predict_family_device(self, d_geno, n_samp: int, pedigree, prior, d_h1, d_h2, d_prob, d_support, d_matching=None,
                              d_dosage=None, vote_method: int = 1, stream=None):
        """Device-pointer form of :meth:`predict_family`: ``pedigree`` and ``prior`` are HOST arrays (the library checks them
        and orders the work by them), the other pointer arguments are ints (``tensor.data_ptr()``) or None."""
        ped, pr = self._family_args(pedigree, prior, int(n_samp))
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_family_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), _as_ptr(ped), _as_ptr(pr), p(d_h1), p(d_h2), p(d_prob),
            p(d_support), p(d_matching), p(d_dosage), p(stream)))

    def predict_device(self, d_geno, n_samp: int, vote_method: int = 1, d_h1=None, d_h2=None, d_prob=None,
                       d_matching=None, d_dosage=None, d_postprob=None, stream=None):
        """Device-pointer form; arguments are ints (``tensor.data_ptr()``) or None."""
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_device(
            self.handle, p(d_geno), int(n_samp), int(vote_method), p(d_h1), p(d_h2), p(d_prob), p(d_matching),
            p(d_dosage), p(d_postprob), p(stream)))

    def batch_limit(self) -> int:
        """Samples one call of the partial entry takes (``hibag_hip_model_batch_limit``)."""
        return int(_lib.lib().hibag_hip_model_batch_limit(self.handle))

    def predict_partial_device(self, d_geno, n_samp: int, d_partial, stream=None):
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_predict_partial_device(self.handle, p(d_geno), int(n_samp), p(d_partial), p(stream)))

    def finish_device(self, d_partial, n_samp: int, d_h1=None, d_h2=None, d_prob=None, d_matching=None,
                      d_dosage=None, d_postprob=None, stream=None):
        p = _dev_ptr
        _lib.check(_lib.lib().hibag_hip_finish_device(
            self.handle, p(d_partial), int(n_samp), p(d_h1), p(d_h2), p(d_prob), p(d_matching), p(d_dosage),
            p(d_postprob), p(stream)))


class GroupsPlan:
    """``hibag_hip_groups``: partitions of one model's alleles as the lists the group finish walks, on the model's device.
    ``group_of`` int32 [n_part, n_hla]; ``levels[q]`` the number of groups of partition q, ``offsets`` [n_part + 1] where its
    groups start in a row of the dosage output, ``n_level`` their total."""

    def __init__(self, model: HlaAttrBagClass, group_of):
        g = np.asarray(group_of)
        if g.dtype.kind not in "iu" or g.ndim != 2 or g.shape[1] != model.obj.n_hla:
            raise ValueError(f"group_of must be an integer matrix [n_part, n_hla = {model.obj.n_hla}]")
        self.group_of = np.ascontiguousarray(g, np.int32)
        if not np.array_equal(self.group_of, g):
            raise ValueError("group_of holds ids an int32 cannot hold")
        self.model = model
        self._h = None
        h = C.c_void_p()
        _lib.check(_lib.lib().hibag_hip_groups_create(model.handle, int(g.shape[0]), _as_ptr(self.group_of), C.byref(h)))
        self._h = h
        self.n_part = int(g.shape[0])
        lv = np.empty(self.n_part, np.int32)
        _lib.check(_lib.lib().hibag_hip_groups_levels(self._h, _as_ptr(lv)))
        self.levels = lv
        self.offsets = np.concatenate([[0], np.cumsum(lv, dtype=np.int64)])
        self.n_level = int(self.offsets[-1])

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise HibagHipError(-4, "the plan has been closed")
        return self._h

    def tile(self):
        """(samples per workgroup of the finish kernel, whether their posteriors are staged in LDS) as the launcher decides
        them now (``HIBAG_GROUPS_NO_LDS=1`` in the environment forces the direct path)."""
        lds = C.c_int(0)
        t = int(_lib.lib().hibag_hip_groups_tile(self.handle, C.byref(lds)))
        if t < 0:
            _lib.check(t)
        return t, bool(lds.value)

    def close(self):
        if getattr(self, "_h", None) is not None:
            _lib.lib().hibag_hip_groups_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_slice(n_samp: int, n_models: int, i: int):
    """(first, count) of replica i's contiguous sample slice (``hibag_hip_multi_slice``; host arithmetic only)."""
    a, b = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().hibag_hip_multi_slice(int(n_samp), int(n_models), int(i), C.byref(a), C.byref(b)))
    return a.value, b.value


def plan_total(gx: int, n_item: int, slots_few: int, slots_many: int, k_req: int, vote: bool = False, all_fp4: bool = False,
               split: bool = False) -> dict:
    """Tests only: pass 1's launch arithmetic with every input given (``hibag_hip_test_plan_total``; no device): the
    ``p1_*`` plan fields of ``hibag_hip_launch_info`` without the prefix."""
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().hibag_hip_test_plan_total(int(gx), int(n_item), int(slots_few), int(slots_many), int(k_req),
                                                    int(bool(vote)), int(bool(all_fp4)), int(bool(split)), C.byref(info)))
    d = info.as_dict()
    return {k: d["p1_" + k] for k in ("n", "slots", "k", "n_whole", "rest", "stride", "grid", "many")}


def plan_accum(nx: int, slots: int, k_req: int) -> dict:
    """Tests only: pass 2's launch arithmetic (``hibag_hip_test_plan_accum``; no device): the ``p2_*`` plan fields."""
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().hibag_hip_test_plan_accum(int(nx), int(slots), int(k_req), C.byref(info)))
    d = info.as_dict()
    return {k: d["p2_" + k] for k in ("nx", "sx", "k", "n_whole", "grid")}


def predict_multi(models: Sequence[HlaAttrBagClass], genomat: np.ndarray, vote_method: int = 1, want_dosage: bool = True,
                  want_prob: bool = False) -> dict:
    """``hibag_hip_predict_multi``: one cohort over several replicas of a model (one per device, one host thread each,
    contiguous sample slices, no collective) -- the counterpart of ``hlaPredict(cl=<cluster>)`` (``R/HIBAG.R:764-808``)."""
    if not models:
        raise ValueError("no models given")
    obj = models[0].obj
    g = np.ascontiguousarray(genomat, np.int32)
    if g.ndim != 2 or g.shape[1] != obj.n_snp:
        raise ValueError("genomat must be [n_samp, n.snp] int32")
    n = g.shape[0]
    out = dict(h1=np.zeros(n, np.int32), h2=np.zeros(n, np.int32),
               prob=np.zeros(n, np.float64), matching=np.zeros(n, np.float64))
    if want_dosage:
        out["dosage"] = np.zeros((n, obj.n_hla), np.float64)
    if want_prob:
        out["postprob"] = np.zeros((n, obj.n_cell), np.float64)
    hs = (C.c_void_p * len(models))(*[m.handle for m in models])
    _lib.check(_lib.lib().hibag_hip_predict_multi(
        hs, len(models), _as_ptr(g), n, int(vote_method), _as_ptr(out["h1"]), _as_ptr(out["h2"]),
        _as_ptr(out["prob"]), _as_ptr(out["matching"]), _as_ptr(out.get("dosage")), _as_ptr(out.get("postprob"))))
    return out


class ShardGroup:
    """``hibag_hip_shard_group``: the shards of one model, each on its device, merged per batch by ONE RCCL all-reduce
    issued by the library itself (``hibag_amd/csrc/hibag_shard.hip``).  ``devices``: one entry per shard (a device may
    repeat: its shards are added up on it before the all-reduce)."""

    def __init__(self, model: HlaAttrBagClass, devices: Sequence[int]):
        if not devices:
            raise ValueError("no devices given")
        self.obj = model.obj
        self.shards = [model.shard(i, len(devices), int(d)) for i, d in enumerate(devices)]
        hs = (C.c_void_p * len(self.shards))(*[m.handle for m in self.shards])
        h = _lib.lib().hibag_hip_shard_group_new(hs, len(self.shards))
        if not h:
            msg = _lib.lib().hibag_hip_last_error().decode()
            for m in self.shards:
                m.close()
            raise HibagHipError(-2, msg)
        self._h = C.c_void_p(h)

    @property
    def ranks(self) -> int:
        return int(_lib.lib().hibag_hip_shard_group_ranks(self._h))

    @property
    def allreduces(self) -> int:
        return int(_lib.lib().hibag_hip_shard_group_allreduces(self._h))

    def predict_raw(self, genomat: np.ndarray, want_dosage: bool = True, want_prob: bool = False) -> dict:
        g = np.ascontiguousarray(genomat, np.int32)
        if g.ndim != 2 or g.shape[1] != self.obj.n_snp:
            raise ValueError("genomat must be [n_samp, n.snp] int32")
        n = g.shape[0]
        out = dict(h1=np.zeros(n, np.int32), h2=np.zeros(n, np.int32), prob=np.zeros(n, np.float64), matching=np.zeros(n, np.float64))
        if want_dosage:
            out["dosage"] = np.zeros((n, self.obj.n_hla), np.float64)
        if want_prob:
            out["postprob"] = np.zeros((n, self.obj.n_cell), np.float64)
        _lib.check(_lib.lib().hibag_hip_shard_group_predict(
            self._h, _as_ptr(g), n, _as_ptr(out["h1"]), _as_ptr(out["h2"]), _as_ptr(out["prob"]), _as_ptr(out["matching"]),
            _as_ptr(out.get("dosage")), _as_ptr(out.get("postprob"))))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None:
            _lib.lib().hibag_hip_shard_group_free(self._h)
            self._h = None
            for m in self.shards:
                m.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hlaModelFromObj(obj: HlaAttrBagObj, device: Optional[int] = None) -> HlaAttrBagClass:
    """``hlaModelFromObj`` (``R/HIBAG.R:1135-1178``)."""
    if not isinstance(obj, HlaAttrBagObj):
        raise TypeError("inherits(obj, \"hlaAttrBagObj\") is not TRUE")
    return HlaAttrBagClass(obj, device)


def hlaModelToObj(model: HlaAttrBagClass) -> HlaAttrBagObj:
    """``hlaModelToObj`` (``R/HIBAG.R:1041-1062``)."""
    if not isinstance(model, HlaAttrBagClass):
        raise TypeError("inherits(model, \"hlaAttrBagClass\") is not TRUE")
    return model.obj


def hlaClose(model: HlaAttrBagClass) -> None:
    model.close()


class HlaAlleleClass:
    """``hlaAlleleClass`` as returned by ``hlaPredict`` (``R/HIBAG.R:729-748``): ``locus``, ``sample_id``, ``allele1`` /
    ``allele2`` (lists of allele names, ``None`` = NA), ``prob``, ``matching``, ``assembly``, ``dosage`` [n_hla, n_samp] (rows =
    ``hla.allele``), ``postprob`` [n_cell, n_samp] (rows = ``pair_names``), and the calls as 0-based allele indices ``h1`` /
    ``h2`` (NA = INT_MIN).

    R builds the two name columns with one vectorised gather, ``object$hla.allele[H1 + 1L]`` -- pointers into its string
    cache.  The counterpart here is a categorical: a result of ``hlaPredict`` keeps the indices and the model's allele
    names (``levels``) and makes the lists the first time ``allele1`` / ``allele2`` is read, so that a caller who wants the
    indices, the probabilities or the dosages does not pay 2 x n_samp Python objects per call."""

    def __init__(self, locus: str, sample_id: List, allele1: Optional[List[Optional[str]]] = None,
                 allele2: Optional[List[Optional[str]]] = None, prob: Optional[np.ndarray] = None,
                 matching: Optional[np.ndarray] = None, assembly: str = "unknown", dosage: Optional[np.ndarray] = None,
                 postprob: Optional[np.ndarray] = None, pair_names: Optional[List[str]] = None,
                 h1: Optional[np.ndarray] = None, h2: Optional[np.ndarray] = None, levels: Optional[Sequence[str]] = None):
        if (allele1 is None or allele2 is None) and (h1 is None or h2 is None or levels is None):
            raise TypeError("HlaAlleleClass needs allele1 and allele2, or h1, h2 and levels")
        self.locus, self.sample_id = locus, sample_id
        self._allele1, self._allele2, self._levels = allele1, allele2, levels
        self.prob, self.matching, self.assembly = prob, matching, assembly
        self.dosage, self.postprob = dosage, postprob
        self.pair_names = [] if pair_names is None else pair_names
        self.h1, self.h2 = h1, h2

    def _names_of(self, h: np.ndarray) -> List[Optional[str]]:
        n = len(self._levels)
        lv = np.empty(n + 1, dtype=np.object_)
        lv[:n] = list(self._levels)
        lv[n] = None
        return lv.take(np.where(np.asarray(h) == NA_INTEGER, n, h)).tolist()

    @property
    def allele1(self) -> List[Optional[str]]:
        if self._allele1 is None:
            self._allele1 = self._names_of(self.h1)
        return self._allele1

    @allele1.setter
    def allele1(self, v):
        self._allele1 = v

    @property
    def allele2(self) -> List[Optional[str]]:
        if self._allele2 is None:
            self._allele2 = self._names_of(self.h2)
        return self._allele2

    @allele2.setter
    def allele2(self, v):
        self._allele2 = v

    def __repr__(self):
        return f"HlaAlleleClass(locus={self.locus!r}, {len(self.sample_id)} samples, assembly={self.assembly!r})"


def _pair_names(alleles: Sequence[str]) -> List[str]:
    # outer(a, a, paste, sep="/")[lower.tri(, diag=TRUE)] (R/HIBAG.R:746-747): column-major
    # lower triangle = for h1, for h2 >= h1: a[h2]/a[h1] -- the posterior vector's order
    return [f"{alleles[j]}/{alleles[i]}" for i in range(len(alleles)) for j in range(i, len(alleles))]


def _snp_ids(obj, match_type: str) -> List:
    """``hlaSNPID`` (``R/DataUtilities.R:512-524``)."""
    pos = [None if p is None else (int(p) if float(p).is_integer() else float(p)) for p in (obj.snp_position if obj.snp_position is not None else [])]
    if match_type == "Position":
        return pos
    if match_type == "Pos+Allele":
        return [f"{p}-{a}" for p, a in zip(pos, obj.snp_allele)]
    if match_type == "RefSNP+Position":
        return [f"{i}-{p}" for i, p in zip(obj.snp_id, pos)]
    if match_type == "RefSNP":
        return list(obj.snp_id)
    raise ValueError("'arg' should be one of \"Position\", \"Pos+Allele\", \"RefSNP+Position\", \"RefSNP\"")


def _model_pair_names(model: "HlaAttrBagClass") -> List[str]:
    """:func:`_pair_names` of the model's alleles, made once per model (P = nHLA(nHLA+1)/2 strings)."""
    names = model.__dict__.get("_pair_names")
    if names is None:
        names = model.__dict__["_pair_names"] = _pair_names(model.obj.hla_allele)
    return list(names)


_TYPES = ("response+dosage", "response", "prob", "response+prob")
_VOTES = ("prob", "majority")


def _as_integer(g: np.ndarray) -> np.ndarray:
    """``as.integer(snp)`` for a numeric matrix (``R/HIBAG.R:715``): int32 in the array's OWN memory order, NA / NaN /
    anything an int cannot hold -> ``NA_integer_``.  An int32 array is returned as it is -- no copy."""
    g = np.asarray(g)
    if g.dtype == np.int32:
        return g
    if g.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            gi = g.astype(np.int32, order="K")
        bad = ~((g > -2147483648.0) & (g < 2147483648.0))         # NaN, +-inf, out of range: whatever the cast made of them
        if bad.any():
            gi[bad] = NA_INTEGER
        return gi
    if g.dtype.kind in "iub":
        if g.dtype.itemsize < 4 or g.dtype.kind == "b":
            return g.astype(np.int32, order="K")
        big = (g > 2147483647) | (g < -2147483647)
        gi = g.astype(np.int32, order="K")
        if big.any():
            gi[big] = NA_INTEGER
        return gi
    raise TypeError("is.numeric(snp) is not TRUE")


def _predict_matrix(model: "HlaAttrBagClass", family: str, g: np.ndarray, sel: Optional[np.ndarray], flip: Optional[np.ndarray],
                    args: tuple, vote_method: int, **want) -> dict:
    """``PredictHLA`` on the matrix ``g`` [SNP, sample] of an ``hlaSNPGenoClass`` (or the numeric matrix handed to
    ``hlaPredict``) WITHOUT building a second matrix on the host: row ``sel[k]`` holds model SNP k (-1 = absent, ``None`` =
    row k), ``flip[k]`` reverses its allele count -- both applied on the device while the genotypes are packed.  The entry
    follows the array's memory: column-major (R's own order: the transpose view is the C side's sample-major matrix) ->
    ``hibag_hip_predict`` / ``_mapped``; row-major (numpy's default) -> ``hibag_hip_predict_snp_major``.  Bit-identical.
    ``family``: "" for the six outputs of ``PredictHLA`` (``want``: ``want_dosage`` / ``want_prob``), "topk" or "draw" for the
    list entries (``args``: their own arguments, ``(k,)`` or ``(n, seed)``) -- the ``predict_*`` methods of that family."""
    stem = "predict_" + family if family else "predict"
    g = _as_integer(g)
    if flip is not None and not np.any(flip):
        flip = None
    if g.flags.f_contiguous:
        cohort = g.T                          # a view: [n_samp, cohort SNPs], C-contiguous
        if sel is None and flip is None:
            return getattr(model, stem if family else "predict_raw")(cohort, *args, vote_method, **want)
        if sel is None:
            sel = np.arange(model.obj.n_snp, dtype=np.int32)
        return getattr(model, stem + "_mapped")(cohort, sel, flip, *args, vote_method, **want)
    if not g.flags.c_contiguous:
        g = np.ascontiguousarray(g)
    return getattr(model, stem + "_snp_major")(g, sel, flip, *args, vote_method, **want)


class _Resolved(NamedTuple):
    """What ``snp`` resolves to (:func:`_resolve_snp`)."""
    route: str                       # "cohort", "bed" or "matrix"
    plan: object                     # the SNP matching's plan (None: a numeric matrix in model order)
    sample_id: Sequence
    assembly: str
    n_samp: int
    mat: Optional[np.ndarray]        # route "matrix": [SNP, sample] ...
    sel: Optional[np.ndarray]        # ... the row of each model SNP (None: row k) ...
    flip: Optional[np.ndarray]       # ... and which allele counts to reverse (None: none)


def _resolve_snp(obj: HlaAttrBagObj, snp, what: str, match_type: str, allele_check: bool, same_strand: bool, verbose: bool,
                 verbose_match: bool) -> _Resolved:
    """The ``snp`` argument of ``hlaPredict`` / ``hlaPredictTopK`` / ``hlaPredictDraws`` resolved to a route -- a resident
    cohort, a lazily opened BED file, a numeric matrix or vector, an :class:`HlaSNPGeno` with SNP matching -- around the
    verbose header (``what``: the line that says what is predicted)."""
    out = sys.stdout
    if verbose:
        s = list(obj.hla_allele)
        if len(s) > 3:
            s = s[:3] + ["..."]
        n_c = len(obj.classifiers)
        print(f"HIBAG model for HLA-{obj.hla_locus}:\n    {n_c} individual classifier{'s' if n_c > 1 else ''}\n"
              f"    {len(obj.snp_id)} SNPs\n    {obj.n_hla} unique HLA alleles: {', '.join(s)}", file=out)
        print("Prediction:\n    " + what, file=out)

    plan = mat = sel = flip = None
    if isinstance(snp, HlaDeviceCohort):
        # extension: the genotypes are resident on the device (hibag_amd/cohort.py); the SNP matching / strand check runs on
        # the cohort's annotation, with allele frequencies from counts made on the device
        route = "cohort"
        plan = snp.plan_for(obj, match_type, allele_check, same_strand, verbose, verbose_match)
        geno_sampid = list(snp.sample_id)
    elif isinstance(snp, HlaBEDGeno):
        # extension: the genotypes stay in the PLINK BED file; the SNP matching / strand check
        # (R/HIBAG.R:550-686) runs on the annotation and the device decodes the file directly
        from .snpmatch import plan_snps_for_predict
        route = "bed"
        plan = plan_snps_for_predict(obj, snp, snp.allele_freq, match_type, allele_check, same_strand,
                                     verbose, verbose_match)
        geno_sampid = list(snp.sample_id)
    elif not isinstance(snp, HlaSNPGeno):
        route = "matrix"
        g = np.asarray(snp)
        if g.dtype.kind not in "iufb":
            raise TypeError("is.numeric(snp) is not TRUE")
        if g.ndim == 1:
            if g.shape[0] != obj.n_snp:
                raise ValueError("length(snp) == object$n.snp is not TRUE")
            g = g.reshape(-1, 1)
        elif g.ndim != 2 or g.shape[0] != obj.n_snp:
            raise ValueError("nrow(snp) == object$n.snp is not TRUE")
        geno_sampid = range(1, g.shape[1] + 1)
        mat = g
    else:
        # the SNP matching / strand check (R/HIBAG.R:550-686) decides on the annotation; the rows are
        # picked and flipped on the device while the genotypes are packed (hibag_hip_predict_mapped / _snp_major)
        from .snpmatch import _row_afreq, plan_snps_for_predict
        route = "matrix"
        mat = np.asarray(snp.genotype)
        if mat.ndim != 2:
            raise ValueError("'snp$genotype' must be a matrix [n.snp, n.samp]")
        plan = plan_snps_for_predict(obj, snp, lambda rows: _row_afreq(_as_integer(mat[rows])), match_type,
                                     allele_check, same_strand, verbose, verbose_match)
        geno_sampid = snp.sample_id
        if len(geno_sampid) != mat.shape[1]:
            raise ValueError("length(snp$sample.id) == ncol(snp$genotype) is not TRUE")
        sel = None if plan.identity else plan.sel
        flip = plan.flip if (plan.flip is not None and np.any(plan.flip)) else None

    n_samp = len(geno_sampid) if mat is None else mat.shape[1]
    if verbose:
        print(f"# of samples: {n_samp}", file=out)
        print(f"Kernel target: {_kernel_info or 'hip'}", file=out)
    return _Resolved(route, plan, geno_sampid, "auto-silent" if plan is None else plan.assembly, n_samp, mat, sel, flip)


def _predict_resolved(model: "HlaAttrBagClass", snp, r: _Resolved, family: str, args: tuple, vote_method: int, **want) -> dict:
    """The call of the route ``snp`` resolved to, on the model's own device (``family``, ``args``, ``want``:
    :func:`_predict_matrix`)."""
    stem = "predict_" + family if family else "predict"
    if r.route == "cohort":
        return getattr(model, stem + "_cohort")(snp, snp.rows_of(r.plan.sel), r.plan.flip, *args, vote_method, **want)
    if r.route == "bed":
        col = np.where(r.plan.sel >= 0, snp.bed_index[np.maximum(r.plan.sel, 0)], -1)
        return getattr(model, stem + "_bed")(snp.bed_fn, snp.n_bed_samp, snp.n_bed_snp, col, r.plan.flip, *args, vote_method,
                                             **want)
    return _predict_matrix(model, family, r.mat, r.sel, r.flip, args, vote_method, **want)


def _warn_no_prediction(na_cnt: int) -> None:
    if na_cnt > 0:   # R/HIBAG.R:811-815
        import warnings
        warnings.warn(f"No prediction output{'s' if na_cnt > 1 else ''} for {na_cnt} individual"
                      f"{'s' if na_cnt > 1 else ''} (possibly due to missing SNPs).", stacklevel=2)     # (the caller's own warning)


def hlaPredict(object: HlaAttrBagClass, snp: Union[HlaSNPGeno, HlaBEDGeno, np.ndarray], cl=False,
               type: str = "response+dosage", vote: str = "prob", allele_check: bool = True,
               match_type: str = "Position", same_strand: bool = False, verbose: bool = True,
               verbose_match: bool = True):
    """``hlaPredict`` (``R/HIBAG.R:481-818``).

    ``snp`` is an :class:`HlaSNPGeno` or a numeric matrix [n.snp, n.samp] (or a
    vector of length n.snp) laid out like the R argument; also a lazily opened BED file (:class:`HlaBEDGeno`) or a cohort
    resident on the model's device (:class:`HlaDeviceCohort`).  ``cl``: the reference takes a
    ``parallel`` cluster and spreads contiguous sample slices over its workers
    (``R/HIBAG.R:764-808``); here a list of device indices does the same over the GPUs of
    the node (``hibag_hip_predict_multi``: one replica and one host thread per device, no
    collective, results identical to one device).  ``False`` / ``None`` / a thread count:
    the model's own device processes the whole cohort.
    Returns :class:`HlaAlleleClass`, or for ``type="prob"`` the posterior matrix
    [n_cell, n_samp] like the reference.

    Cost: like the reference (``R/HIBAG.R:715-748``: one ``.Call`` and O(1) R-level work per cohort besides the result's
    data frame) the host side does nothing per sample in the interpreter and copies no matrix: the genotypes go to the
    device from the caller's own memory in either memory order, SNP selection and allele flips happen on the device, and
    ``dosage`` / ``postprob`` are returned as [row, sample] VIEWS of the C side's sample-major output -- R's own memory
    order for those matrices.  What `bench.py` reports as ``api_inclusive``.
    """
    if not isinstance(object, HlaAttrBagClass):
        raise TypeError("inherits(object, \"hlaAttrBagClass\") is not TRUE")
    if type not in _TYPES:
        raise ValueError("'arg' should be one of " + ", ".join(f'"{t}"' for t in _TYPES))
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    vote_method = _VOTES.index(vote) + 1
    obj = object.obj
    r = _resolve_snp(obj, snp, "based on the averaged posterior probabilities" if vote_method == 1
                     else "by voting from all individual classifiers", match_type, allele_check, same_strand, verbose, verbose_match)
    geno_sampid, assembly, mat, sel, flip = r.sample_id, r.assembly, r.mat, r.sel, r.flip

    want_prob = type in ("prob", "response+prob")
    want_dosage = type != "response"
    devices = list(cl) if isinstance(cl, (list, tuple)) else None
    if devices is not None:
        # a device list: validated up front (an index out of range used to surface as ENODEV from deep inside replicate())
        n_dev = int(_lib.lib().hibag_hip_device_count())
        bad = [d for d in devices if not isinstance(d, (int, np.integer)) or isinstance(d, bool) or not (0 <= int(d) < n_dev)]
        if not devices or bad:
            raise ValueError(f"'cl' must be a non-empty list of HIP device indices below {n_dev}: {cl!r}")
        if r.route == "cohort":
            raise ValueError("hlaPredict(cl = [devices]) takes a genotype matrix or an hlaSNPGenoClass; a resident cohort "
                             "(HlaDeviceCohort) lives on one device: predict there, with cl = False")
        if r.route == "bed":
            # the BED route decodes on ONE device (hibag_hip_predict_bed); silently ignoring the list would not be what
            # the caller asked for
            raise ValueError("hlaPredict(cl = [devices]) takes a genotype matrix or an hlaSNPGenoClass; for a lazily opened BED "
                             "file (hlaBED2Geno(lazy=True)) predict on one device, or load the genotypes first (hlaBED2Geno())")
    if devices is not None:
        # several devices: hibag_hip_predict_multi slices ONE sample-major matrix in model order over the replicas.  R's memory
        # order with the model's own SNPs is that matrix already; anything else is put in that form on the host (the model's
        # few hundred rows of the cohort)
        g = _as_integer(mat)
        if sel is None and flip is None and g.flags.f_contiguous:
            genomat = g.T
        else:
            idx = np.arange(obj.n_snp) if sel is None else np.asarray(sel)
            rows = g[np.maximum(idx, 0)]
            if flip is not None:
                fl = np.asarray(flip, bool)[:, None]
                rows = np.where(fl & (rows >= 0) & (rows <= 2), 2 - rows, rows)
            rows[idx < 0] = NA_INTEGER
            genomat = np.ascontiguousarray(rows.T, np.int32)
        cache = object.__dict__.setdefault("_replicas", {})
        reps = []
        for d in devices:
            key = (int(d), len([r for r in reps if r[0] == int(d)]))      # (several replicas on one device are allowed)
            if key not in cache:
                cache[key] = object.replicate(int(d))
            reps.append((int(d), cache[key]))
        rv = predict_multi([r for _, r in reps], genomat, vote_method, want_dosage=want_dosage, want_prob=want_prob)
    else:
        rv = _predict_resolved(object, snp, r, "", (), vote_method, want_dosage=want_dosage, want_prob=want_prob)

    if type == "prob":
        res = rv["postprob"].T                # [n_cell, n_samp]: a view of the sample-major output = R's memory order
        with np.errstate(invalid="ignore"):
            na_cnt = int(np.count_nonzero(rv["postprob"].sum(axis=1) <= 0))
    else:
        h1, h2 = rv["h1"], rv["h2"]
        na_cnt = int(np.count_nonzero((h1 == NA_INTEGER) | (h2 == NA_INTEGER)))
        # (allele1 / allele2: object$hla.allele[H1 + 1L] (R/HIBAG.R:729-736), made from h1 / h2 and the levels when first read)
        res = HlaAlleleClass(locus=obj.hla_locus, sample_id=list(geno_sampid), h1=h1, h2=h2, levels=obj.hla_allele,
                             prob=rv["prob"], matching=rv["matching"], assembly=assembly,
                             dosage=(rv["dosage"].T if type != "response" else None),
                             postprob=(rv["postprob"].T if want_prob else None),
                             pair_names=_model_pair_names(object) if want_prob else [])

    _warn_no_prediction(na_cnt)
    return res
