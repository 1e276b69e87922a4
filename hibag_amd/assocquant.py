"""``hlaAssocQuant``: allele association tests of a quantitative trait (the continuous-``y`` half of ``R/Association.R``),
with max-T permutation p-values.

For a real-valued trait ``y`` (a titre, an expression level, age at onset) and covariates ``c1 ... cq``, every test of the
analysis -- each allele of the typed cohort and, with ``groups``, each level of every partition of the alleles -- is one
``lm(y ~ h + c1 + ... + cq)``: an estimate, its confidence interval and t-test p-value per ``h`` column and the F statistic
of the ``h`` columns together, beside the reference's class columns: the mean of ``y`` per genotype class (``avg.``) and
Welch's t-test (``ttest.p``) or the one-way ANOVA (``anova.p``) between the classes.  ``n_perm`` Freedman-Lane permutations of
the residual trait give ``perm_p`` (pointwise) and ``perm_p_adj`` (family-wise, single-step max-T) on the F statistic.  With
the constant and the covariates orthonormalised, all tests under all permutations are one real-valued Gram matrix, int8
feature rows x FP64 residual rows, on the FP64 matrix cores (``hibag_hip_assoc_quant_*``).  The result is defined exactly
 and does not depend on panel sizes or on how the permutations are split over calls.

Not built: ``use_prob`` weights (and exchangeability under weights), other families, interaction terms, and permutations for
``hlaAssocGlm``."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _attach_perm, _check_model, _check_perm, _Plan, _ptr
from .assocglm import MAX_COVAR, Z975, _condition_list, _condition_tests, _design, _DeviceGlm
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

FLAG_RANK = 2                      # HIBAG_HIP_QUANT_RANK


class _DeviceQuant(_DeviceGlm):
    """The tests of one cohort on the device, with a quantitative trait on them (``hibag_hip_quant``)."""

    _q = None

    def quant(self, y: np.ndarray, covar: Optional[np.ndarray]) -> None:
        """The trait ``y`` [n_kept] and the covariates [q, n_kept]; ValueError for collinear covariates."""
        y = np.ascontiguousarray(y, np.float64)
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        L = _lib.lib()
        self.quant_close()
        self.n_basis = 1 + (0 if covar is None else covar.shape[0])
        self._q = L.hibag_hip_assoc_quant_new(self._h, _ptr(y), _ptr(covar), self.n_basis - 1)
        if not self._q:
            msg = L.hibag_hip_last_error().decode("utf-8", "replace")
            if "collinear" in msg:
                raise ValueError("the covariates are collinear")
            raise _lib.HibagHipError(-1, msg)

    def quant_close(self) -> None:
        if self._q:
            _lib.lib().hibag_hip_assoc_quant_free(self._q)
            self._q = None

    def close(self) -> None:
        self.quant_close()
        super().close()

    def quant_classes(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
        """(cnt int64, S1, S2 [n_tests, 3], ybar)."""
        cnt = np.empty((self.n_tests, 3), np.int64)
        S1, S2, ybar = np.empty((self.n_tests, 3)), np.empty((self.n_tests, 3)), np.empty(1)
        _lib.check(_lib.lib().hibag_hip_assoc_quant_classes(self._q, _ptr(cnt), _ptr(S1), _ptr(S2), _ptr(ybar)))
        return cnt, S1, S2, float(ybar[0])

    def quant_observed(self):
        """(proj [rows, n_basis], g [rows], rr, stat [n_tests], flags [n_tests])."""
        proj, g, rr = np.empty((self.n_rows, self.n_basis)), np.empty(self.n_rows), np.empty(1)
        stat, flags = np.empty(self.n_tests), np.empty(self.n_tests, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_quant_observed(self._q, _ptr(proj), _ptr(g), _ptr(rr), _ptr(stat), _ptr(flags)))
        return proj, g, float(rr[0]), stat, flags

    def quant_permute(self, seed: int, perm0: int, n_perm: int) -> Tuple[np.ndarray, np.ndarray]:
        max_stat = np.empty(n_perm, np.float64)
        count = np.empty(self.n_tests, np.int64)
        _lib.check(_lib.lib().hibag_hip_assoc_quant_permute(self._q, seed, perm0, n_perm, _ptr(max_stat), _ptr(count)))
        return max_stat, count

    def quant_perm_rows(self, seed: int, perm0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n_kept), np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_quant_perm_rows(self._q, seed, perm0, n, _ptr(out)))
        return out

    def quant_gram_ms(self) -> float:
        ms = _lib.C.c_double(0.0)
        _lib.check(_lib.lib().hibag_hip_assoc_quant_gram_ms(self._q, _lib.C.byref(ms)))
        return float(ms.value)


# ---- the regularised incomplete beta function ----------------------------------------------------------------------------
def _betacf(a: float, b: float, x: float) -> float:
    """The continued fraction of I_x(a, b) by the modified Lentz method (converges fast for x < (a + 1) / (a + b + 2))."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def betainc(a: float, b: float, x: float) -> float:
    """The regularised incomplete beta function I_x(a, b) for a, b > 0 and 0 <= x <= 1 (NaN for NaN): the continued
    fraction, reflected to 1 - I_{1-x}(b, a) where x > (a + 1) / (a + b + 2)."""
    if math.isnan(x) or math.isnan(a) or math.isnan(b):
        return math.nan
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    log_front = a * math.log(x) + b * math.log1p(-x) - (math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b))
    if x < (a + 1.0) / (a + b + 2.0):
        return math.exp(log_front) * _betacf(a, b, x) / a
    return 1.0 - math.exp(log_front) * _betacf(b, a, 1.0 - x) / b


def _t_p(t: float, df: float) -> float:
    """The two-sided tail of Student's t: I_x(df / 2, 1 / 2) with x = df / (df + t^2)."""
    if math.isnan(t) or math.isnan(df):
        return math.nan
    if math.isinf(t):
        return 0.0
    return betainc(df / 2.0, 0.5, df / (df + t * t))


def _f_p(f: float, d1: float, d2: float) -> float:
    """The upper tail of F(d1, d2): I_x(d2 / 2, d1 / 2) with x = d2 / (d2 + d1 f)."""
    if math.isnan(f):
        return math.nan
    if math.isinf(f):
        return 0.0
    return betainc(d2 / 2.0, d1 / 2.0, d2 / (d2 + d1 * f))


def _class_columns(model: str, cnt: np.ndarray, S1: np.ndarray, S2: np.ndarray, ybar: float, n: int):
    """(avg [T, k], ttest_p or None, anova_p or None) from the class sums; the classes of
    ``additive`` are the dosages 0, 1, 2."""
    T = len(cnt)
    kinds = (0, 1, 2) if model in ("additive", "genotype") else (0, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = ybar + S1 / cnt
        var = (S2 - S1 * S1 / cnt) / (cnt - 1)
    avg[cnt == 0] = np.nan
    p = np.full(T, np.nan)
    eps = 2.0 ** -52
    for t in range(T):
        c = cnt[t]
        if model in ("dominant", "recessive"):
            if c[0] < 2 or c[1] < 2:
                continue
            v0, v1 = var[t, 0] / c[0], var[t, 1] / c[1]
            se = math.sqrt(v0 + v1)
            if se < 10.0 * eps * max(abs(avg[t, 0]), abs(avg[t, 1])):
                continue
            tt = (avg[t, 0] - avg[t, 1]) / se
            df = se ** 4 / (v0 * v0 / (c[0] - 1) + v1 * v1 / (c[1] - 1))
            p[t] = _t_p(tt, df)
        else:
            used = [d for d in kinds if c[d] > 0]
            kk = len(used)
            if kk < 2 or n - kk < 1:
                continue
            ssw = sum(S2[t, d] - S1[t, d] * S1[t, d] / c[d] for d in used)
            tot = sum(S1[t, d] for d in used)
            ssb = sum(S1[t, d] * S1[t, d] / c[d] for d in used) - tot * tot / n
            with np.errstate(divide="ignore", invalid="ignore"):
                F = float((np.float64(ssb) / (kk - 1)) / (np.float64(ssw) / (n - kk)))
            p[t] = _f_p(F, kk - 1, n - kk)
    two = model in ("dominant", "recessive")
    return avg[:, :len(kinds)], (p if two else None), (None if two else p)


QUANT_CLASS_NAMES = {"dominant": ("[-/-]", "[-/h,h/h]"), "additive": ("[-/-]", "[-/h]", "[h/h]"),
                     "recessive": ("[-/-,-/h]", "[h/h]"), "genotype": ("[-/-]", "[-/h]", "[h/h]")}


class HlaAssocQuantResult:
    """The table of ``hlaAssocQuant``, one entry per test in the order of ``hlaAssocTest``.  ``class_names`` are the genotype
    classes of the model (the dosages 0 / 1 / 2 for ``additive``); ``counts`` int64 and ``avg`` [n_test, k] the samples and the
    mean of ``y`` per class (NaN where empty); ``ttest_p`` (``dominant``, ``recessive``: Welch) or ``anova_p`` (``additive``,
    ``genotype``), the other one ``None``.  ``h_names`` are the ``h`` columns, ``("h",)`` or ``("h1", "h2")``; ``est``, ``se``,
    ``lower``, ``upper``, ``pval`` are [n_test, d] over them, NaN where a column was not fitted; ``stat`` is the F statistic of
    the ``h`` columns (t squared for one column), ``stat_p`` its tail, ``rss`` the residual sum of squares, ``df`` the residual
    degrees of freedom, ``flags`` bit 1 a test that was not fitted.  With permutations ``perm_p``, ``perm_p_adj``,
    ``max_stat`` [n_perm], ``n_perm`` and ``seed``.  ``covariates`` names the basis columns after the constant."""

    def __init__(self, model: str, locus: str, name: List[str], counts, avg, ttest_p, anova_p, h_names: Tuple[str, ...], est, se, lower,
                 upper, pval, stat, stat_p, rss, df, flags, covariates: List[str], n_samp: int, n_excluded: int, n_perm: int = 0,
                 seed: Optional[int] = None, perm_p=None, perm_p_adj=None, max_stat=None):
        self.model, self.locus, self.name = model, locus, name
        self.class_names = QUANT_CLASS_NAMES[model]
        self.counts, self.avg, self.ttest_p, self.anova_p = counts, avg, ttest_p, anova_p
        self.h_names, self.est, self.se, self.lower, self.upper, self.pval = h_names, est, se, lower, upper, pval
        self.stat, self.stat_p, self.rss, self.df, self.flags = stat, stat_p, rss, df, flags
        self.covariates, self.n_samp, self.n_excluded = covariates, n_samp, n_excluded
        self.n_perm, self.seed = n_perm, seed
        self.perm_p, self.perm_p_adj, self.max_stat = perm_p, perm_p_adj, max_stat

    def to_table(self) -> Dict[str, np.ndarray]:
        """The columns under the reference's names: the class counts, ``avg.`` per class, ``ttest.p`` or ``anova.p``, then per
        ``h`` column ``h.est``, ``h.2.5%``, ``h.97.5%``, ``h.pval``, then ``perm.p`` and ``perm.p.adj`` when there were
        permutations; the rows are ``name``."""
        out: Dict[str, np.ndarray] = {}
        for j, c in enumerate(self.class_names):
            out[c] = self.counts[:, j]
        for j, c in enumerate(self.class_names):
            out["avg." + c] = self.avg[:, j]
        if self.ttest_p is not None:
            out["ttest.p"] = self.ttest_p
        else:
            out["anova.p"] = self.anova_p
        for j, h in enumerate(self.h_names):
            out[f"{h}.est"], out[f"{h}.2.5%"] = self.est[:, j], self.lower[:, j]
            out[f"{h}.97.5%"], out[f"{h}.pval"] = self.upper[:, j], self.pval[:, j]
        if self.n_perm > 0:
            out["perm.p"], out["perm.p.adj"] = self.perm_p, self.perm_p_adj
        return out

    def __repr__(self):
        return (f"HlaAssocQuantResult({self.model!r}, {len(self.name)} tests, {len(self.covariates)} covariates, "
                f"{self.n_samp} samples, {self.n_perm} permutations)")


def _fit_columns(model: str, n: int, nb: int, cnt, proj, g, rr: float, stat, flags):
    """The host columns of the observed run: est, se [T, d], rss, df [T]."""
    T = len(cnt)
    d = 2 if model == "genotype" else 1
    est, se = np.full((T, d), np.nan), np.full((T, d), np.nan)
    rss, df = np.full(T, np.nan), np.full(T, np.nan)
    for t in range(T):
        if flags[t] & FLAG_RANK:
            continue
        c = cnt[t]
        if model == "genotype" and c[1] > 0 and c[2] > 0:
            p1, p2 = proj[2 * t], proj[2 * t + 1]
            a11, a22 = float(c[1]) - float(np.cumsum(p1 * p1)[-1]), float(c[2]) - float(np.cumsum(p2 * p2)[-1])
            a12 = -float(np.cumsum(p1 * p2)[-1])
            det = a11 * a22 - a12 * a12
            g1, g2 = float(g[2 * t]), float(g[2 * t + 1])
            m = ((a22 * (g1 * g1) - ((2.0 * a12) * g1) * g2) + a11 * (g2 * g2)) / det
            df[t] = n - nb - 2
            rss[t] = rr - m
            s2 = rss[t] / df[t]
            est[t] = (a22 * g1 - a12 * g2) / det, (a11 * g2 - a12 * g1) / det
            if s2 > 0:
                se[t] = math.sqrt(s2 * a22 / det), math.sqrt(s2 * a11 / det)
            continue
        if model == "genotype":
            col = 0 if c[1] > 0 else 1
            row, xx = 2 * t + col, float(c[1] + c[2])
        else:
            col, row, xx = 0, t, float(c[1] + 4 * c[2])
        pr = proj[row]
        sxx = xx - float(np.cumsum(pr * pr)[-1])
        m = float(g[row]) * float(g[row]) / sxx
        df[t] = n - nb - 1
        rss[t] = rr - m
        s2 = rss[t] / df[t]
        est[t, col] = float(g[row]) / sxx
        if s2 > 0:
            se[t, col] = math.sqrt(s2 / sxx)
    return est, se, rss, df


def hlaAssocQuant(hla: HlaAlleleClass, y: Sequence, covariates=None, model: str = "dominant", prob_threshold: float = float("nan"),
                  groups: Optional[HlaAlleleGroups] = None, condition: Optional[Sequence[str]] = None, n_perm: int = 0,
                  seed: Optional[int] = None, use_prob: bool = False, _backend=None) -> HlaAssocQuantResult:
    """Association tests of the alleles of ``hla`` with the quantitative trait ``y`` (``hlaAssocTest`` of the reference
    with a continuous ``y``: ``t.test`` / ``aov`` and ``glm(..., family = gaussian)``), on the device.

    * ``hla``, ``prob_threshold``, ``groups`` and the list of tests: as ``hlaAssocTest``.  ``y``: one float per sample; a
      non-finite value of a kept sample is a ValueError.
    * ``covariates``, ``condition``: as ``hlaAssocGlm``; at most 12 columns together.  Collinear columns are a ValueError.
    * ``model``: the ``h`` column of a test, one value per SAMPLE: ``dominant`` carrier 0 / 1, ``additive`` the dosage
      0 / 1 / 2, ``recessive`` homozygous 0 / 1, ``genotype`` the dummies ``h1`` (het) and ``h2`` (hom).  The class columns
      (no covariates involved, as in the reference) are per class of that value: Welch's ``ttest_p`` for two classes,
      ``anova_p`` over the non-empty classes for ``additive`` and ``genotype``.
    * ``n_perm > 0``: Freedman-Lane permutations of the residual trait under ``seed`` (drawn and reported when ``None``);
      ``perm_p`` and the family-wise ``perm_p_adj`` as ``hlaAssocTest``'s, on the F statistic ``stat``.

    A test whose column is constant over the kept samples, or lies in the span of the covariates, has flag bit 1 and NaN;
    ``genotype``: a dummy that nobody carries is left out (its columns NaN), and a test with nobody WITHOUT the allele has
    bit 1.  Not built: ``use_prob`` weights (``use_prob=True`` is a ValueError: a weighted permutation test needs
    exchangeability under weights), other families, interactions, and permutations for
    ``hlaAssocGlm``.  (``_backend``: the tests' seam, a class with the interface of ``_DeviceQuant``.)"""
    _check_model(model)
    if use_prob:
        raise ValueError("use_prob is not built for hlaAssocQuant (DESIGN.md section 25, 'Not built'): threshold the calls with prob_threshold")
    n_perm, seed = _check_perm(n_perm, seed)
    if not isinstance(hla, HlaAlleleClass):
        raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
    n_all = len(hla.sample_id)
    try:
        yv = np.asarray(y, np.float64).ravel()
    except (TypeError, ValueError):
        raise ValueError("y must be numeric") from None
    if len(yv) != n_all:
        raise ValueError(f"'hla' and 'y' must have the same length ({n_all} samples, {len(yv)} values of y)")
    plan = _Plan(hla, None, prob_threshold, groups)
    yk = np.ascontiguousarray(yv[plan.sel])
    if not np.isfinite(yk).all():
        raise ValueError("y has a missing or non-finite value: subset the samples first")
    cov_names, cov, _ = _design(plan, hla, covariates, False)
    condition = _condition_list(condition)
    per = 2 if model == "genotype" else 1
    cond_rows, cond_names = _condition_tests(plan, condition, per)
    cov_names += cond_names
    q = len(cov_names)
    if q > MAX_COVAR:
        raise ValueError(f"{q} covariate columns ({len(condition)} conditioned tests included); at most {MAX_COVAR}")
    n, nb = plan.n_samp, q + 1
    if n - nb - per < 1:
        raise ValueError(f"{n} samples leave no residual degree of freedom with {q} covariate columns")

    backend = _DeviceQuant if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        for row in cond_rows:
            cov = np.concatenate([cov, dev.feature_rows(per * row, per).astype(np.float64)])
        dev.quant(yk, cov)
        d_cnt, d_S1, d_S2, ybar = dev.quant_classes()
        d_proj, d_g, rr, d_stat, d_flags = dev.quant_observed()
        if n_perm > 0:
            max_stat, d_count = dev.quant_permute(seed, 1, n_perm)

    d_avg, d_tp, d_ap = _class_columns(model, d_cnt, d_S1, d_S2, ybar, n)
    d_est, d_se, d_rss, d_df = _fit_columns(model, n, nb, d_cnt, d_proj, d_g, rr, d_stat, d_flags)
    pick, known = plan.spread, np.array(plan.row) >= 0
    counts = pick(d_cnt[:, :d_avg.shape[1]], 0).astype(np.int64)
    counts[~known, 0] = n
    avg = pick(d_avg)
    avg[~known, 0] = ybar
    est, se, rss, df = pick(d_est), pick(d_se), pick(d_rss), pick(d_df)
    stat = pick(d_stat)
    flags = pick(d_flags, FLAG_RANK).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        tval = est / se
    pval = np.array([_t_p(float(tv), float(dd)) for tv, dd in zip(tval.ravel(), np.repeat(df, per))]).reshape(tval.shape)
    n_col = np.isfinite(est).sum(axis=1)
    stat_p = np.array([_f_p(float(s), float(k), float(dd)) if k > 0 else math.nan for s, k, dd in zip(stat, n_col, df)])
    res = HlaAssocQuantResult(model, hla.locus, plan.names, counts, avg, None if d_tp is None else pick(d_tp),
                              None if d_ap is None else pick(d_ap), ("h1", "h2") if per == 2 else ("h",), est, se, est - Z975 * se,
                              est + Z975 * se, pval, stat, stat_p, rss, df, flags, cov_names, plan.n_samp, plan.n_excluded)
    if n_perm > 0:
        _attach_perm(res, plan, stat, max_stat, d_count, n_perm, seed)
    return res


__all__ = ["HlaAssocQuantResult", "hlaAssocQuant"]
