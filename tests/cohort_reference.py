"""The resident form of a cohort (hibag_amd/csrc/hibag_k_cohort.h) stated in numpy.

2 bits per genotype, SNP-major, one row per SNP: PLINK's codes (2 -> 00, missing -> 01, 1 -> 10, 0 -> 11), four samples per
byte from the low bits up, rows ``stride`` bytes apart with ``stride`` = ceil(n_samp / 4) rounded up to 16; every slot
behind the last sample holds the missing code.  Anything outside 0..2 is missing."""
import numpy as np

NA = -2147483648


def stride_of(n_samp: int) -> int:
    return ((n_samp + 3) // 4 + 15) // 16 * 16


def pack(geno: np.ndarray, snp_major: bool = True) -> np.ndarray:
    """uint8 [n_snp, stride] from the int matrix [n_snp, n_samp] (``snp_major``) or [n_samp, n_snp]."""
    g = np.asarray(geno)
    if not snp_major:
        g = g.T
    n_snp, n_samp = g.shape
    stride = stride_of(n_samp)
    code = np.full((n_snp, 4 * stride), 1, np.uint8)
    real = code[:, :n_samp]
    real[g == 2] = 0
    real[g == 1] = 2
    real[g == 0] = 3
    q = code.reshape(n_snp, stride, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def codes(rows: np.ndarray) -> np.ndarray:
    """The 2-bit codes of packed rows, uint8 [n_snp, 4 * stride]."""
    rows = np.asarray(rows, np.uint8)
    return np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(rows.shape[0], -1)


def unpack(rows: np.ndarray, n_samp: int) -> np.ndarray:
    """int32 [n_snp, n_samp]: 0 / 1 / 2, NA for the missing code."""
    return np.array([2, NA, 1, 0], np.int32)[codes(rows)[:, :n_samp]]


def counts(rows: np.ndarray):
    """Per row the number of called genotypes (int32) and their sum (int64), over the whole stride (the padding is missing)."""
    c = codes(rows)
    val = np.array([2, 0, 1, 0], np.int64)[c]
    return (c != 1).sum(axis=1).astype(np.int32), val.sum(axis=1).astype(np.int64)


def allele_freq(rows: np.ndarray) -> np.ndarray:
    """``rowMeans(genotype, na.rm=TRUE) * 0.5`` from :func:`counts`, with the expression of ``snpmatch._row_afreq``."""
    n_valid, total = counts(rows)
    cnt = n_valid.astype(np.int64)
    tot = total.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, tot / cnt, np.nan) * 0.5


def random_geno(rng, n_snp: int, n_samp: int) -> np.ndarray:
    """int32 [n_snp, n_samp] of 0 / 1 / 2 with NA and a few other out-of-range values (all of them missing)."""
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.int32)
    m = rng.random((n_snp, n_samp))
    g[m < 0.10] = NA
    g[(m >= 0.10) & (m < 0.12)] = 3
    g[(m >= 0.12) & (m < 0.14)] = -1
    return g


def canonical(g: np.ndarray) -> np.ndarray:
    """What survives packing: anything outside 0..2 becomes NA."""
    g = np.asarray(g)
    return np.where((g >= 0) & (g <= 2), g, NA).astype(np.int32)
