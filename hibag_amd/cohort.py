"""A cohort's genotypes resident on the device, and multi-locus typing on it.

A real run types ONE cohort at every locus (published models ship as a list per locus, ``modellist$A``, ``$B``, ...) and
then asks again: the k best pairs, the other vote method, a second ancestry's model.  ``hlaPredict`` takes the raw
genotypes anew on every call -- 4 bytes per genotype up the bus, a decode per model, a BED file read again per locus.

:class:`HlaDeviceCohort` keeps them on the device at 2 bits per genotype (``hibag_hip_cohort``, ``include/hibag_hip.h``:
the payload of a SNP-major PLINK BED file, so matrices and files share the decode the BED route already has) together with
the annotation SNP matching needs.  ``hlaPredict`` and ``hlaPredictTopK`` accept it as ``snp``; :func:`hlaPredictLoci`
types a cohort with a list of models.  Every field of every result is bit for bit what ``hlaPredict(model, snp, ...)``
returns for the object the cohort was made from.
"""

from __future__ import annotations

import ctypes as C
import os
from collections.abc import Mapping
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import HibagHipError
from .bed import HlaBEDGeno
from .model import HlaAttrBagObj, HlaSNPGeno


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HlaDeviceCohort:
    """The genotypes of ``snp`` -- an :class:`HlaSNPGeno` or a lazily opened :class:`HlaBEDGeno` -- resident on one
    device, with the annotation of an ``hlaSNPGenoClass`` (``sample_id``, ``snp_id``, ``snp_position``, ``snp_allele``,
    ``assembly``).  ``snp_sel`` (indices or a boolean mask) keeps a subset of the object's SNPs, in the given order;
    ``device`` selects the HIP device like ``hlaModelFromObj`` (default: the calling thread's current one).

    A matrix goes up in slabs and is packed on the device (anything outside 0..2 is missing, the kernels' rule); a BED
    file's rows are loaded straight from the file.  The object is immutable, usable with any number of models on its
    device, a context manager, and raises ``ValueError`` once closed."""

    def __init__(self, snp: Union[HlaSNPGeno, HlaBEDGeno], snp_sel=None, device: Optional[int] = None):
        if not isinstance(snp, (HlaSNPGeno, HlaBEDGeno)):
            raise TypeError("'snp' must be an hlaSNPGenoClass (HlaSNPGeno) or a lazily opened BED file (HlaBEDGeno)")
        n_all = len(snp.snp_id)
        if snp_sel is None:
            ann = None
        else:
            ann = np.asarray(snp_sel)
            if ann.dtype == np.bool_:
                if ann.shape != (n_all,):
                    raise ValueError("a boolean 'snp_sel' must have one entry per SNP")
                ann = np.where(ann)[0]
            ann = ann.astype(np.int64)
            if ann.ndim != 1 or (len(ann) and (ann.min() < 0 or ann.max() >= n_all)):
                raise ValueError(f"'snp_sel' must hold SNP indices below {n_all}")
        self._h = None
        self._row_of = None          # annotation index -> resident row (None: the same; -1: not resident)
        self._counts_cache = None
        self._host_afreq = None
        self._build(snp, ann, ann, device)

    @classmethod
    def _partial(cls, snp: Union[HlaSNPGeno, HlaBEDGeno], rows: np.ndarray, host_afreq, device: Optional[int] = None) -> "HlaDeviceCohort":
        """The whole annotation of ``snp`` with only the SNPs ``rows`` (ascending, unique) resident: what
        :func:`hlaPredictLoci` builds for a host-side object once it knows which rows its models use.  The host object is
        at hand for the whole life of such a cohort, so its allele frequencies are the host's own (``host_afreq(rows)``,
        what ``hlaPredict(model, snp)`` consults): the SNP matching is the same computation, not an equivalent one."""
        self = cls.__new__(cls)
        self._h = None
        self._counts_cache = None
        self._host_afreq = host_afreq
        rows = np.asarray(rows, np.int64)
        self._row_of = np.full(len(snp.snp_id), -1, np.int64)
        self._row_of[rows] = np.arange(len(rows))
        self._build(snp, None, rows, device)
        return self

    def _build(self, snp, ann: Optional[np.ndarray], resident: Optional[np.ndarray], device: Optional[int]) -> None:
        def pick(v):
            return list(v) if ann is None else [v[i] for i in ann]
        self.sample_id = list(snp.sample_id)
        self.snp_id = pick(snp.snp_id)
        self.snp_position = None if snp.snp_position is None else (
            np.asarray(snp.snp_position, np.float64) if ann is None else np.asarray(snp.snp_position, np.float64)[ann])
        self.snp_allele = pick(snp.snp_allele)
        self.assembly = snp.assembly
        L = _lib.lib()
        if device is not None:
            _lib.check(L.hibag_hip_set_device(int(device)))
        rows32 = None if resident is None else np.ascontiguousarray(resident, np.int32)
        if isinstance(snp, HlaBEDGeno):
            idx = np.ascontiguousarray(snp.bed_index if resident is None else np.asarray(snp.bed_index)[resident], np.int32)
            h = L.hibag_hip_cohort_from_bed(os.fsencode(snp.bed_fn), int(snp.n_bed_samp), int(snp.n_bed_snp), _ptr(idx), len(idx))
            n_rows = len(idx)
            self.uploaded_bytes = ((int(snp.n_bed_samp) + 3) // 4) * n_rows if snp.mode != 0 else None
        else:
            from .hibag import _as_integer
            mat = np.asarray(snp.genotype)
            if mat.ndim != 2:
                raise ValueError("'snp$genotype' must be a matrix [n.snp, n.samp]")
            if len(snp.sample_id) != mat.shape[1]:
                raise ValueError("length(snp$sample.id) == ncol(snp$genotype) is not TRUE")
            g = _as_integer(mat)
            n_snp, n_samp = g.shape
            if g.flags.c_contiguous:
                snp_major, ld = 1, max(n_samp, 1)
            elif g.flags.f_contiguous:
                g = g.T                           # a view: [n_samp, n_snp] in C order, R's own memory
                snp_major, ld = 0, max(n_snp, 1)
            else:
                g = np.ascontiguousarray(g)
                snp_major, ld = 1, max(n_samp, 1)
            n_rows = n_snp if rows32 is None else len(rows32)
            h = L.hibag_hip_cohort_new(_ptr(g), snp_major, ld, n_samp, n_snp, _ptr(rows32), n_rows)
            self.uploaded_bytes = 4 * n_samp * n_rows
        if not h:
            raise HibagHipError(-1, L.hibag_hip_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)
        self._n_samp = int(L.hibag_hip_cohort_n_samp(self._h))
        self._n_rows = int(L.hibag_hip_cohort_n_snp(self._h))

    # -- the handle ---------------------------------------------------------------------------------------------------
    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise ValueError("the cohort has been closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            _lib.lib().hibag_hip_cohort_free(self._h)
            self._h = None

    def __enter__(self) -> "HlaDeviceCohort":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_samp(self) -> int:
        return self._n_samp

    @property
    def n_snp(self) -> int:
        """SNPs of the annotation (all of them resident unless the cohort was made by ``hlaPredictLoci`` for its own use)."""
        return len(self.snp_id)

    @property
    def nbytes(self) -> int:
        """Device memory of the resident rows."""
        return int(_lib.lib().hibag_hip_cohort_bytes(self.handle))

    def device(self) -> int:
        return int(_lib.lib().hibag_hip_cohort_device(self.handle))

    def __repr__(self):
        state = "closed" if self._h is None else f"{self._n_rows} SNP rows resident"
        return f"HlaDeviceCohort({len(self.sample_id)} samples, {len(self.snp_id)} SNPs, assembly={self.assembly!r}, {state})"

    # -- what SNP matching asks of the genotypes ----------------------------------------------------------------------
    def rows_of(self, sel: np.ndarray) -> np.ndarray:
        """Resident row of each annotation index in ``sel`` (-1 stays -1)."""
        sel = np.asarray(sel, np.int64)
        if self._row_of is None:
            return sel
        rows = np.where(sel >= 0, self._row_of[np.maximum(sel, 0)], -1)
        if np.any((sel >= 0) & (rows < 0)):
            raise ValueError("the cohort does not hold every SNP this model matches")
        return rows

    def snp_counts(self):
        """Per resident row: the number of called genotypes (int32) and their sum (int64), counted on the device."""
        if self._counts_cache is None:
            h = self.handle
            n_valid = np.empty(self._n_rows, np.int32)
            total = np.empty(self._n_rows, np.int64)
            _lib.check(_lib.lib().hibag_hip_cohort_snp_counts(h, _ptr(n_valid), _ptr(total)))
            self._counts_cache = (n_valid, total)
        self.handle      # (raises once closed, cache or not)
        return self._counts_cache

    def allele_freq(self, rows) -> np.ndarray:
        """A-allele frequency of the SNPs ``rows`` -- ``rowMeans(genotype, na.rm=TRUE) * 0.5`` -- from the device's exact
        counts, formed with the host expression of ``snpmatch._row_afreq`` so that the strand check decides as it does
        on the host matrix.  The counts follow the kernels' rule: a stray value outside 0..2 that is not NA (3, -1) is
        missing here, whereas ``_row_afreq`` on the host matrix adds it up; for matrices of 0 / 1 / 2 / NA and for BED
        files the two are the same doubles."""
        self.handle
        if self._host_afreq is not None:
            self.rows_of(np.asarray(rows, np.int64))
            return self._host_afreq(rows)
        r = self.rows_of(np.asarray(rows, np.int64))
        n_valid, total = self.snp_counts()
        cnt = n_valid[r].astype(np.int64)
        tot = total[r].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cnt > 0, tot / cnt, np.nan) * 0.5

    def plan_for(self, obj: HlaAttrBagObj, match_type: str, allele_check: bool, same_strand: bool, verbose: bool,
                 verbose_match: bool):
        """``hlaPredict``'s SNP matching of ``obj`` against this cohort (``snpmatch.plan_snps_for_predict``)."""
        from .snpmatch import plan_snps_for_predict
        self.handle
        return plan_snps_for_predict(obj, self, self.allele_freq, match_type, allele_check, same_strand, verbose, verbose_match)


_TYPES = ("response+dosage", "response", "prob", "response+prob")
_VOTES = ("prob", "majority")


def _models_by_locus(models) -> List:
    """``[(locus, model)]`` in the caller's order; raises on an empty or ill-typed collection and on a locus given twice."""
    from .hibag import HlaAttrBagClass
    if isinstance(models, (HlaAttrBagClass, HlaAttrBagObj)):
        raise TypeError("'models' must be a mapping or a sequence of models, not a single model")
    if isinstance(models, Mapping):
        items = [(k, m) for k, m in models.items()]
        keyed = True
    elif isinstance(models, (list, tuple)):
        items = [(None, m) for m in models]
        keyed = False
    else:
        raise TypeError("'models' must be a mapping {locus: model} or a sequence of models")
    if not items:
        raise ValueError("'models' is empty")
    out, seen = [], set()
    for k, m in items:
        if not isinstance(m, (HlaAttrBagClass, HlaAttrBagObj)):
            raise TypeError("every element of 'models' must be an hlaAttrBagClass (HlaAttrBagClass) or an hlaAttrBagObj "
                            f"(HlaAttrBagObj): {type(m).__name__}")
        locus = str(k) if keyed else str(m.hla_locus)
        if locus in seen:
            raise ValueError(f"locus {locus!r} is given more than once in 'models'")
        seen.add(locus)
        out.append((locus, m))
    return out


def hlaPredictLoci(models, snp, type: str = "response+dosage", vote: str = "prob", allele_check: bool = True,
                   match_type: str = "Position", same_strand: bool = False, verbose: bool = True) -> Dict[str, object]:
    """``hlaPredict`` of one cohort with every model of ``models`` -- the loop a multi-locus run makes -- over genotypes
    that go to the device once.

    ``models``: a mapping ``{locus: model}`` or a sequence of models (keyed by their ``hla_locus``), each an
    :class:`HlaAttrBagClass` or an :class:`HlaAttrBagObj` (put on the device for the call and closed afterwards).
    ``snp``: an :class:`HlaDeviceCohort` (used as it is), or an :class:`HlaSNPGeno` / :class:`HlaBEDGeno`: every model's
    SNP matching is planned on the annotation first, then only the rows some model uses become a temporary cohort, freed
    at the end; each locus is then matched again by its own run, against the same host frequencies.  The other arguments
    are ``hlaPredict``'s.  The loci run one after another in the order of ``models``; the result is ``{locus: what hlaPredict(model, snp, ...) returns}`` in that order, bit for bit."""
    from .hibag import HlaAttrBagClass, _as_integer, hlaPredict
    loci = _models_by_locus(models)
    if type not in _TYPES:
        raise ValueError("'arg' should be one of " + ", ".join(f'"{t}"' for t in _TYPES))
    if vote not in _VOTES:
        raise ValueError("'arg' should be one of \"prob\", \"majority\"")
    if not isinstance(snp, (HlaDeviceCohort, HlaSNPGeno, HlaBEDGeno)):
        raise TypeError("'snp' must be an HlaDeviceCohort, an hlaSNPGenoClass (HlaSNPGeno) or a lazily opened BED file (HlaBEDGeno)")

    opened: List = []
    cohort = snp if isinstance(snp, HlaDeviceCohort) else None
    try:
        on_device = []
        for locus, m in loci:
            if isinstance(m, HlaAttrBagObj):
                m = HlaAttrBagClass(m, cohort.device() if cohort is not None else None)
                opened.append(m)
            on_device.append((locus, m))
        if cohort is None:
            # plan every locus on the annotation (silently: each locus prints its own matching when it runs), then make the
            # rows some model uses resident
            from .snpmatch import _row_afreq, plan_snps_for_predict
            if isinstance(snp, HlaBEDGeno):
                afreq = snp.allele_freq
            else:
                mat = np.asarray(snp.genotype)
                if mat.ndim != 2:
                    raise ValueError("'snp$genotype' must be a matrix [n.snp, n.samp]")

                def afreq(rows):
                    return _row_afreq(_as_integer(mat[rows]))
            # (a first, silent pass only to learn the rows: each locus's own run matches again on the cohort, with the same
            # frequencies, and prints and warns what hlaPredict prints and warns)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                plans = [plan_snps_for_predict(m.obj, snp, afreq, match_type, allele_check, same_strand, False, False)
                         for _, m in on_device]
            used = np.unique(np.concatenate([p.sel[p.sel >= 0] for p in plans]))
            cohort = HlaDeviceCohort._partial(snp, used, afreq, on_device[0][1].device())
        out: Dict[str, object] = {}
        for locus, m in on_device:
            out[locus] = hlaPredict(m, cohort, type=type, vote=vote, allele_check=allele_check, match_type=match_type,
                                    same_strand=same_strand, verbose=verbose)
        return out
    finally:
        if cohort is not None and cohort is not snp:
            cohort.close()
        for m in opened:
            m.close()
