"""``hlaAssocHaplo``: covariate-adjusted score tests of a case / control trait on multi-locus haplotypes.

Whether ``A*01:01~B*08:01~DRB1*03:01`` carries risk that none of its alleles carries alone is a question about haplotypes.
``hlaHaplotypes`` estimates them from imputed calls, with every sample's posterior over its phased states; this entry tests
them.  With ``dosage="expected"`` the regressor of a haplotype is every sample's EXPECTED number of copies under that
posterior (``HlaHaplotypeResult.dosage``, a real number in [0, 2]), so phase and imputation uncertainty shrink the regressor
instead of being rounded away; with ``dosage="best"`` it is the 0 / 1 / 2 count of the called pair, which is ``hlaAssocScore`` on
``haplo.as_alleles(min_freq)`` as it is.  The base model, the weighted basis, the sign stream, the residual panels, the
statistics kernel and min-P are those of ``hlaAssocScore``; the real-valued rows go through
``hibag_hip_assoc_rscore_sets`` and the FP64 kernels of ``csrc/hibag_k_rscore.h`` (section 30).

This is the EXPECTATION-SUBSTITUTION score test: the expected dosage is the regressor and the variance is the model's.  It is
not Schaid's ``haplo.score`` variance, which adds the posterior variance of the dosage given the genotypes; for well-imputed
haplotypes the two are close, and under the null both are valid to first order.

Not built: ``use_prob``, quantitative traits, dominant and recessive codings, haplotype x haplotype interactions."""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .assoc import _check_perm, _Plan
from .assocglm import COV0, FLAG_MAXIT, FLAG_RANK, MAX_COVAR, _base_model, _check_fit_control, _condition_list, _design
from .assocscore import MAX_ROWS, HlaAssocScoreResult, _DeviceScore, _min_p, chisq_sf_array, hlaAssocScore
from .haplo import HlaHaplotypeResult

DOSAGES = ("expected", "best")


class HlaAssocHaploResult(HlaAssocScoreResult):
    """The table of ``hlaAssocHaplo``: the columns of :class:`HlaAssocScoreResult`, one entry per haplotype with ``freq >=
    min_freq`` named ``A*01:01~B*08:01`` (or the one global test ``"omnibus"``), plus ``freq`` (the haplotype's estimated
    frequency) and ``mean_dosage`` (the mean of its regressor over the samples that entered; NaN for the omnibus test).
    ``dosage`` says which regressor was used."""

    dosage = "expected"
    freq = None
    mean_dosage = None

    def to_table(self):
        out = {"freq": self.freq, "mean.dosage": self.mean_dosage}
        out.update(super().to_table())
        return out

    def __repr__(self):
        return (f"HlaAssocHaploResult({self.dosage!r}, {len(self.name)} {'set' if self.omnibus else 'haplotypes'}, "
                f"{len(self.base['name']) - 1} covariate columns, {self.n_samp} samples with {self.n_case} cases, {self.n_perm} replicates)")


def rare_row(rows: np.ndarray) -> np.ndarray:
    """``(2.0 - d_0) - d_1 - ...`` over the rows in order, one rounding per subtraction: the dosage of every haplotype that is
    not among the rows."""
    out = np.full(rows.shape[1], 2.0)
    for r in rows:
        out = out - r
    return out


def _selected(haplo: HlaHaplotypeResult, min_freq: float) -> np.ndarray:
    return np.flatnonzero(np.asarray(haplo.freq) >= min_freq)


def hlaAssocHaplo(haplo: HlaHaplotypeResult, y: Sequence, covariates=None, min_freq: float = 0.01, dosage: str = "expected",
                  omnibus: bool = False, condition: Optional[Sequence[str]] = None, n_perm: int = 0, seed: Optional[int] = None,
                  maxit: int = 25, epsilon: float = 1e-8, _backend=None) -> HlaAssocHaploResult:
    """Score tests of ``y ~ d_h + covariates`` against ``y ~ covariates``, logistic, for every haplotype h of ``haplo`` with
    ``freq >= min_freq``, with family-wise p-values by multiplier resampling, on the device.

    * ``haplo``: a result of ``hlaHaplotypes``; ``y``, ``covariates``, ``maxit``, ``epsilon``, ``n_perm``, ``seed``: as
      ``hlaAssocScore``, per sample of ``haplo.sample_id``.  The samples ``hlaHaplotypes`` left out do not enter.
    * ``dosage="expected"``: the regressor is ``haplo.dosage`` -- ``hlaHaplotypes(..., dosage_min_freq=f)`` with ``f <=
      min_freq``; a result without it, or with ``f > min_freq``, is a ValueError.  ``dosage="best"``: the copies of the
      haplotype in the called pair, ``hlaAssocScore(haplo.as_alleles(min_freq), model="additive", ...)``.
    * ``omnibus=False``: one test with one degree of freedom per selected haplotype.  ``omnibus=True``: one global test on one
      set -- the selected haplotypes without the most frequent one, plus the row ``rare`` = 2 minus all selected dosages
      (under ``best`` the rows are the 0 / 1 / 2 counts of the called pair); more than 30 columns is a ValueError.
    * ``condition``: names of selected haplotypes whose rows join the covariates (real-valued under ``expected``); at most 12
      covariate columns together.

    This is the expectation-substitution score test: the expected dosage is the regressor and the variance comes from the
    model; it is not Schaid's ``haplo.score`` variance with the posterior-variance correction.  (``_backend``: the tests'
    seam, as in ``hlaAssocScore``, with ``score_real_sets``.)"""
    if not isinstance(haplo, HlaHaplotypeResult):
        raise TypeError("'haplo' must be an HlaHaplotypeResult (hlaHaplotypes)")
    if dosage not in DOSAGES:
        raise ValueError(f"dosage must be one of {DOSAGES}")
    if isinstance(min_freq, bool) or not isinstance(min_freq, (int, float, np.floating)) or not (0 <= float(min_freq) <= 1):
        raise ValueError("min_freq must be a number in [0, 1]")
    min_freq, omnibus = float(min_freq), bool(omnibus)
    _check_fit_control(maxit, epsilon)
    n_perm, seed = _check_perm(n_perm, seed)
    condition = _condition_list(condition, "haplotype")
    sel = _selected(haplo, min_freq)
    if len(sel) == 0:
        raise ValueError(f"no haplotype has a frequency of at least {min_freq}")
    names = [haplo.names(int(i)) for i in sel]
    for c in condition:
        if c not in names:
            raise ValueError(f"condition: {c!r} is not a haplotype of this analysis (freq >= min_freq)")
    n_cols = len(sel) if omnibus else 1                    # (omnibus: the selected ones without the first, plus `rare`)
    if n_cols > MAX_ROWS:
        raise ValueError(f"the omnibus test has {n_cols} columns; at most {MAX_ROWS} (raise min_freq)")
    if dosage == "expected":
        if haplo.dosage is None or haplo.dosage_index is None:
            raise ValueError("dosage='expected' needs the dosages of the result: hlaHaplotypes(..., dosage_min_freq=f) with f <= min_freq")
        if min_freq < float(haplo.dosage_min_freq):
            raise ValueError(f"min_freq = {min_freq} is below the result's dosage_min_freq = {haplo.dosage_min_freq}")
    hla = haplo.as_alleles(min_freq)
    freq = np.asarray(haplo.freq, np.float64)[sel]

    if dosage == "best" and not omnibus:
        return _best(haplo, hla, y, covariates, names, freq, condition, n_perm, seed, maxit, epsilon, _backend)

    plan = _Plan(hla, y, float("nan"), None)
    cov_names, cov, _ = _design(plan, hla, covariates, False)
    n_user = len(cov_names)
    if dosage == "expected":
        at = {int(i): r for r, i in enumerate(np.asarray(haplo.dosage_index).tolist())}
        D = np.ascontiguousarray(np.asarray(haplo.dosage, np.float64)[[at[int(i)] for i in sel]][:, plan.sel])   # [selected, kept]
    else:                              # (the omnibus test on the called pairs: their 0 / 1 / 2 counts as rows)
        h1, h2 = np.asarray(hla.h1)[plan.sel], np.asarray(hla.h2)[plan.sel]
        lv = np.arange(len(sel))[:, None]
        D = (h1[None, :] == lv).astype(np.float64) + (h2[None, :] == lv).astype(np.float64)
    if not np.isfinite(D).all():
        raise ValueError("the dosages of the used samples are not finite")
    for c in condition:
        cov = np.concatenate([cov, D[names.index(c)][None, :]])
        cov_names.append(f"h[{c}]")
    q = len(cov_names)
    if q > MAX_COVAR:
        raise ValueError(f"{q} covariate columns ({q - n_user} conditioned columns included); at most {MAX_COVAR}")
    if omnibus:
        rows = np.concatenate([D[1:], rare_row(D)[None, :]])
        sets, out_names = [list(range(len(rows)))], ["omnibus"]
        out_freq, mean = np.array([np.nan]), np.array([np.nan])
    else:
        rows, sets, out_names = D, [[j] for j in range(len(D))], names
        out_freq, mean = freq, D.sum(axis=1) / D.shape[1]

    backend = _DeviceScore if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), None, 0) as dev:       # (the handle: kept samples, y, the stream)
        dev.score(cov, None, int(maxit), float(epsilon))
        b_coef, b_se, b_dev, b_it, b_fl = dev.score_base()
        dev.score_real_sets(rows, sets)
        _, stat, df, flags = dev.score_observed()
        if n_perm > 0:
            max_stat, d_count = dev.score_resample(seed, 1, n_perm)
    if b_fl & FLAG_RANK:
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    stat, df, flags = np.asarray(stat, np.float64), np.asarray(df, np.int32), np.asarray(flags, np.int32)
    score_p = np.full(len(stat), np.nan)
    for d in sorted(set(df[df > 0].tolist())):
        score_p[df == d] = chisq_sf_array(stat[df == d], d)
    base = _base_model(b_coef, b_se, b_dev, b_it, b_fl, [0] + list(range(COV0, COV0 + q)), cov_names)
    res = HlaAssocHaploResult("additive", hla.locus, omnibus, list(out_names), df, stat, score_p, flags, base, plan.n_samp, plan.n_case,
                              plan.n_excluded)
    res.dosage, res.freq, res.mean_dosage = dosage, out_freq, mean
    if n_perm > 0:
        dfs = sorted(set(df[df > 0].tolist()))
        assert max_stat.shape == (n_perm, len(dfs))
        min_p = _min_p(max_stat, dfs)
        nan = np.isnan(stat)
        order = np.sort(min_p[~np.isnan(min_p)])
        count_min = np.searchsorted(order, score_p, side="right")
        res.perm_p = np.where(nan, np.nan, (1 + np.asarray(d_count)) / (n_perm + 1))
        res.perm_p_adj = np.where(nan, np.nan, (1 + count_min) / (n_perm + 1))
        res.max_stat, res.max_stat_df, res.min_p = max_stat, np.array(dfs, np.int32), min_p
        res.n_perm, res.seed = n_perm, seed
    return res


def _best(haplo, hla, y, covariates, names: List[str], freq, condition, n_perm, seed, maxit, epsilon, _backend) -> HlaAssocHaploResult:
    """``dosage="best"`` per haplotype: hlaAssocScore's additive path on the called haplotype pairs, reported per selected
    haplotype.  (The family of ``perm_p_adj`` is hlaAssocScore's: it holds the level ``rare`` too where a sample carries it.)"""
    r = hlaAssocScore(hla, y, covariates, model="additive", condition=condition or None, n_perm=n_perm, seed=seed, maxit=maxit,
                      epsilon=epsilon, _backend=_backend)
    # the tests of hlaAssocScore are the levels carried by a kept sample, in its own order: pick the selected haplotypes
    at = {n: i for i, n in enumerate(r.name)}
    pick = np.array([at.get(n, -1) for n in names], np.int64)
    have = pick >= 0

    def col(a, fill):
        a = np.asarray(a)
        return np.where(have, a[np.maximum(pick, 0)], fill).astype(a.dtype)

    res = HlaAssocHaploResult("additive", hla.locus, False, list(names), col(r.df, 0), col(r.score_stat, np.nan), col(r.score_p, np.nan),
                              col(r.flags, FLAG_RANK | (int(r.base["flags"]) & FLAG_MAXIT)), r.base, r.n_samp, r.n_case, r.n_excluded)
    used = np.flatnonzero(haplo.used)
    lv = {n: i for i, n in enumerate(names)}
    h1, h2 = np.asarray(hla.h1)[used], np.asarray(hla.h2)[used]
    res.dosage, res.freq = "best", freq
    res.mean_dosage = np.array([(np.count_nonzero(h1 == lv[n]) + np.count_nonzero(h2 == lv[n])) / len(used) for n in names])
    if r.n_perm > 0:
        res.perm_p, res.perm_p_adj = col(r.perm_p, np.nan), col(r.perm_p_adj, np.nan)
        res.max_stat, res.max_stat_df, res.min_p, res.n_perm, res.seed = r.max_stat, r.max_stat_df, r.min_p, r.n_perm, r.seed
    return res


__all__ = ["HlaAssocHaploResult", "hlaAssocHaplo"]
