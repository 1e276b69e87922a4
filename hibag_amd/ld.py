"""Linkage disequilibrium around an HLA gene: ``hlaGenoLD`` (``R/HIBAG.R:1399-1446``) and ``hlaLDMatrix``
(``R/HIBAG.R:1453-1541``, the ``draw=FALSE`` result).

Both are r^2 from Gram matrices of small integers over samples, computed on the device as int8 matrix products with
exact int32 sums (``hibag_hip_ld_*``, DESIGN.md "LD").  From the exact sums n, Sx, Sxx, Sy, Syy, Sxy over the samples
used, ``num = n Sxy - Sx Sy``, ``dx = n Sxx - Sx^2``, ``dy = n Syy - Sy^2`` (int64) and ``r2 = num^2 / (dx dy)`` in double,
one rounding per operation; NaN where dx or dy is 0.  R's ``cor(...)^2`` is the same quantity with other roundings.

Stated deviations: a numeric matrix handed to ``hlaGenoLD`` must hold 0/1/2 or NA (R would correlate any dosage), and
``draw=True`` raises ``NotImplementedError`` (this package does not plot)."""

from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .bed import hlaLociInfo
from .hibag import HlaAlleleClass, _as_integer
from .model import NA_INTEGER, HlaSNPGeno


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class _DeviceGeno:
    """Genotypes [n_snp, n_samp] resident on the device (``hibag_hip_ld_geno``), handed over in their own memory order."""

    def __init__(self, g: np.ndarray):
        g = _as_integer(g)
        if g.ndim != 2:
            raise ValueError("the genotypes must be a matrix [SNP, sample]")
        n_snp, n_samp = g.shape
        if g.flags.c_contiguous:
            snp_major = 1
        elif g.flags.f_contiguous:
            snp_major = 0                  # the transpose view is [n_samp][n_snp], C-contiguous
        else:
            g, snp_major = np.ascontiguousarray(g), 1
        self._keep = g
        self.n_snp, self.n_samp = n_snp, n_samp
        L = _lib.lib()
        self._h = L.hibag_hip_ld_geno_new(_ptr(g), n_snp, n_samp, snp_major)
        if not self._h:
            raise _lib.HibagHipError(-1, L.hibag_hip_last_error().decode("utf-8", "replace"))

    def close(self) -> None:
        if self._h:
            _lib.lib().hibag_hip_ld_geno_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def snp_counts(self) -> Tuple[np.ndarray, np.ndarray]:
        n_valid = np.empty(self.n_snp, np.int32)
        s = np.empty(self.n_snp, np.int64)
        _lib.check(_lib.lib().hibag_hip_ld_snp_counts(self._h, _ptr(n_valid), _ptr(s)))
        return n_valid, s

    def matrix(self, snp_idx: np.ndarray) -> Tuple[np.ndarray, int]:
        idx = np.ascontiguousarray(snp_idx, np.int32)
        k = idx.size
        r2 = np.empty((k, k), np.float64)
        n_c = C.c_int(0)
        _lib.check(_lib.lib().hibag_hip_ld_matrix(self._h, _ptr(idx), k, _ptr(r2), C.byref(n_c)))
        return r2, n_c.value

    def gram_ms(self) -> float:
        ms = C.c_double(0)
        _lib.check(_lib.lib().hibag_hip_ld_gram_ms(self._h, C.byref(ms)))
        return ms.value

    def hla(self, a1: np.ndarray, a2: np.ndarray, n_allele: int, want_r2: bool) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        a1 = np.ascontiguousarray(a1, np.int32)
        a2 = np.ascontiguousarray(a2, np.int32)
        ld = np.empty(self.n_snp, np.float64)
        r2 = np.empty((self.n_snp, n_allele), np.float64) if want_r2 else None
        _lib.check(_lib.lib().hibag_hip_ld_hla(self._h, _ptr(a1), _ptr(a2), n_allele, _ptr(ld),
                                               None if r2 is None else _ptr(r2)))
        return ld, r2


def _is_na(v) -> bool:
    return v is None or (isinstance(v, float) and math.isnan(v))


def _numeric_geno(geno) -> np.ndarray:
    """A numeric matrix or vector for ``hlaGenoLD``: int32 [n_snp, n_samp]; NaN and INT_MIN are NA, and every other value
    must be 0, 1 or 2."""
    g = np.asarray(geno)
    if g.dtype.kind not in "iufb":
        raise TypeError("is.numeric(geno) is not TRUE")
    if g.ndim == 1:
        g = g.reshape(1, -1)
    elif g.ndim != 2:
        raise ValueError("geno should be `hlaSNPGenoClass', a vector or a matrix.")
    if g.dtype.kind == "f":
        na = np.isnan(g) | (g == float(NA_INTEGER))
    else:
        na = g == NA_INTEGER
    ok = na | (g == 0) | (g == 1) | (g == 2)
    if not ok.all():
        bad = g[~ok].ravel()[0]
        raise ValueError(f"geno holds {bad!r}: genotypes must be 0, 1, 2 or NA")
    out = np.where(na, NA_INTEGER, g).astype(np.int32, order="K")
    return out


def _hla_indices(hla: HlaAlleleClass) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """The sorted allele names and each sample's two 0-based allele indices (NA_INTEGER where the sample is unusable:
    R's ``allele.mat`` row is NA in every column when allele1 or allele2 is NA)."""
    h1, h2 = list(hla.allele1), list(hla.allele2)
    alleles = sorted({a for a in h1 + h2 if not _is_na(a)})
    pos = {a: i for i, a in enumerate(alleles)}
    n = len(h1)
    i1 = np.full(n, NA_INTEGER, np.int32)
    i2 = np.full(n, NA_INTEGER, np.int32)
    for s in range(n):
        if not _is_na(h1[s]) and not _is_na(h2[s]):
            i1[s], i2[s] = pos[h1[s]], pos[h2[s]]
    return alleles, i1, i2


def _geno_ld_r2(hla: HlaAlleleClass, geno: Union[HlaSNPGeno, np.ndarray, Sequence[float]], want_r2: bool = True
                ) -> Tuple[np.ndarray, Optional[np.ndarray], List[str]]:
    """``hlaGenoLD`` with its per-allele r^2 (for tests): (ld [n_snp], r2 [n_snp, n_allele] or None, allele names)."""
    if not isinstance(hla, HlaAlleleClass):
        raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
    n_hla = len(hla.sample_id)
    if isinstance(geno, HlaSNPGeno):
        if n_hla != len(geno.sample_id):
            raise ValueError("dim(hla$value)[1L] == length(geno$sample.id) is not TRUE")
        if list(hla.sample_id) != list(geno.sample_id):
            # R: hlaAlleleSubset(hla, samp.sel = match(geno$sample.id, hla$value$sample.id))
            hpos = {s: i for i, s in enumerate(hla.sample_id)}
            missing = [s for s in geno.sample_id if s not in hpos]
            if missing:
                raise ValueError(f"sample {missing[0]!r} of geno is not in hla")
            sel = [hpos[s] for s in geno.sample_id]
            h1, h2 = list(hla.allele1), list(hla.allele2)
            hla = HlaAlleleClass(locus=hla.locus, sample_id=list(geno.sample_id), allele1=[h1[i] for i in sel],
                                 allele2=[h2[i] for i in sel])
        g = np.asarray(geno.genotype)
    elif isinstance(geno, (np.ndarray, list, tuple)):
        g = _numeric_geno(geno)
        if g.shape[1] != n_hla:
            raise ValueError(f"dim(hla$value)[1L] == dim(geno)[2L] is not TRUE ({n_hla} HLA samples, {g.shape[1]} genotype columns)")
    else:
        raise TypeError("geno should be `hlaSNPGenoClass', a vector or a matrix.")
    alleles, i1, i2 = _hla_indices(hla)
    if g.shape[0] == 0:
        return np.empty(0), np.empty((0, len(alleles))), alleles
    with _DeviceGeno(g) as dg:
        ld, r2 = dg.hla(i1, i2, len(alleles), want_r2)
    return ld, r2, alleles


def hlaGenoLD(hla: HlaAlleleClass, geno: Union[HlaSNPGeno, np.ndarray, Sequence[float]]) -> np.ndarray:
    """Composite LD between every SNP and the HLA locus: for SNP j the mean over the alleles of r^2 between the SNP's
    genotype and the allele's dosage, each r^2 over the samples with a genotype at j and both alleles known
    (``cor(x, allele.mat, use="pairwise.complete.obs")^2``, ``mean(na.rm=TRUE)``).  The alleles are the sorted unique
    non-NA names of allele1 and allele2; the mean sums the non-NaN r^2 in that order and is NaN if there is none.

    ``geno``: an :class:`HlaSNPGeno` (``hla`` is reordered to its samples; a sample of ``geno`` missing from ``hla`` is a
    ValueError), or a numeric matrix [n_snp, n_samp] / vector [n_samp] of 0, 1, 2 and NA (NaN or INT_MIN); any other value
    is a ValueError.  Returns float64 [n_snp]."""
    return _geno_ld_r2(hla, geno, want_r2=False)[0]


def _check_loci(loci, assembly: str, geno: HlaSNPGeno) -> None:
    if loci is None:
        return
    if isinstance(loci, str):
        loci = [loci]
    asm = geno.assembly if assembly == "auto" else assembly
    info = hlaLociInfo(asm) or {}
    if not all(x in info for x in loci):
        raise ValueError("'loci' should be one of " + ", ".join(info))


def hlaLDMatrix(geno: HlaSNPGeno, loci=None, maf: float = 0.01, assembly: str = "auto", draw: bool = False,
                verbose: bool = True) -> np.ndarray:
    """The SNP x SNP r^2 matrix of ``geno`` after a MAF filter: R's ``cor(t(genotype), use="na.or.complete")^2``.

    * MAF filter when ``maf > 0`` (NaN counts as 0): ``af = (sum / n_called) * 0.5``, ``af = min(af, 1 - af)``, SNPs with
      ``af >= maf`` are kept; a SNP without a called genotype is dropped.
    * ``loci`` is checked against ``hlaLociInfo(assembly)`` and otherwise unused (there is no plot).
    * The samples used are those called at every kept SNP (casewise deletion).
    * Returns float64 [n_kept, n_kept], symmetric, in input SNP order; 0 x 0 when no SNP is kept.
    * The diagonal is 1.0 even for a SNP that is constant over the complete samples (its other entries are NaN), and
      with fewer than two complete samples every entry is NaN, the diagonal included.  These two rules follow R's
      ``cov.c`` as read, not as run.

    ``draw=True`` raises ``NotImplementedError``: this package has no plotting."""
    if not isinstance(geno, HlaSNPGeno):
        raise TypeError('inherits(geno, "hlaSNPGenoClass") is not TRUE')
    if isinstance(maf, bool) or not isinstance(maf, (int, float, np.integer, np.floating)):
        raise TypeError("is.numeric(maf) is not TRUE")
    if not isinstance(draw, (bool, np.bool_)):
        raise TypeError("is.logical(draw) is not TRUE")
    if not isinstance(verbose, (bool, np.bool_)):
        raise TypeError("is.logical(verbose) is not TRUE")
    if draw:
        raise NotImplementedError("hlaLDMatrix(draw=TRUE): this package has no plotting; use draw=False for the matrix")
    _check_loci(loci, assembly, geno)
    maf = float(maf)
    if math.isnan(maf):
        maf = 0.0
    g = np.asarray(geno.genotype)
    n_snp = g.shape[0]
    if n_snp == 0:
        return np.empty((0, 0), np.float64)
    with _DeviceGeno(g) as dg:
        keep = np.arange(n_snp, dtype=np.int32)
        if maf > 0:
            n_valid, s = dg.snp_counts()
            with np.errstate(divide="ignore", invalid="ignore"):
                af = (s / n_valid) * 0.5
                af = np.minimum(af, 1.0 - af)
                ok = af >= maf                          # NaN (no called genotype) -> dropped
            if ok.sum() < n_snp:
                if verbose:
                    print(f"MAF filter (>={maf:.7g}), excluding {n_snp - int(ok.sum())} SNP(s)")
                keep = np.flatnonzero(ok).astype(np.int32)
        r2, _ = dg.matrix(keep)
    return r2


__all__ = ["hlaGenoLD", "hlaLDMatrix"]
