"""``hlaAssocGlm``: covariate-adjusted logistic regression per allele (the ``glm`` half of ``R/Association.R``).

For a case / control trait ``y`` and covariates ``c1 ... cq`` (sex, age, ancestry components), every test of the analysis --
each allele of the typed cohort and, with ``groups``, each level of every partition of the alleles -- is one
``glm(y ~ h + c1 + ... + cq, family = binomial)``: an estimate (log odds ratio, or odds ratio with ``show_or``), its
confidence interval and Wald p-value per ``h`` column, and a likelihood-ratio test against the base model
``y ~ c1 + ... + cq``.  ``condition`` repeats the scan conditioned on earlier hits.  All fits are independent and share the
covariates; they run on the device (``hibag_hip_assoc_glm``), one workgroup per fit, with ``X'WX`` and ``X'Wz`` of every
iteration as one 16 x 16 FP64 matrix-core tile.  The fit is R's ``glm.fit`` restated.  The test of a
whole partition -- all residues of a position at once -- is ``hlaAssocOmnibus`` (assocomni.py).

Not built: other ``family`` values (a quantitative trait with the t-test and ANOVA columns is ``hlaAssocQuant``,
assocquant.py), permutation p-values for this regression (the family-wise p-value of the same tests is ``hlaAssocScore``,
assocscore.py: score tests with multiplier resampling), R's step halving, interaction terms, and ``fisher_p`` of the
genotype model."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _check_model, _DeviceAssoc, _Plan, _chisq_p, _ptr
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

MAX_COVAR = 12                     # HIBAG_HIP_GLM_MAX_COVAR
SLOTS = 16                         # coefficient slots of a fit: 0 intercept, 1 h (het), 2 hom, 3 .. the covariates
COV0 = 3
FLAG_MAXIT, FLAG_RANK, FLAG_BOUNDARY = 1, 2, 4
Z975 = 1.959963984540054           # qnorm(0.975)


class _DeviceGlm(_DeviceAssoc):
    """The tests of one cohort on the device, with the regression entries."""

    def feature_rows(self, row0: int, n_rows: int) -> np.ndarray:
        out = np.empty((n_rows, self.n_kept), np.int8)
        _lib.check(_lib.lib().hibag_hip_assoc_feature_rows(self._h, row0, n_rows, _ptr(out)))
        return out

    def glm(self, covar: Optional[np.ndarray], weight: Optional[np.ndarray], maxit: int, epsilon: float):
        """(coef, se [n_tests + 1, 16], deviance, iterations, flags [n_tests + 1]); covar [q, n_kept], weight [n_kept]."""
        n_fit = self.n_tests + 1
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        weight = None if weight is None else np.ascontiguousarray(weight, np.float64)
        coef, se = np.empty((n_fit, SLOTS)), np.empty((n_fit, SLOTS))
        dev, it, fl = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_glm(self._h, _ptr(covar), 0 if covar is None else covar.shape[0], _ptr(weight), maxit,
                                                  epsilon, _ptr(coef), _ptr(se), _ptr(dev), _ptr(it), _ptr(fl)))
        return coef, se, dev, it, fl


def _wald(est: np.ndarray, se: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lower, upper, pval) of ``confint.default`` and ``summary.glm``: est -+ qnorm(0.975) se, erfc(|est / se| / sqrt 2)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.abs(est / se)
    pval = np.array([math.erfc(v / math.sqrt(2.0)) if not math.isnan(v) else math.nan for v in z.ravel()]).reshape(z.shape)
    return est - Z975 * se, est + Z975 * se, pval


class HlaAssocGlmResult:
    """The table of ``hlaAssocGlm``, one entry per test in the order of ``hlaAssocTest``.  ``h_names`` are the ``h`` columns,
    ``("h",)`` or, for the genotype model, ``("h1", "h2")`` (het, hom); ``est``, ``se``, ``lower``, ``upper``, ``pval`` are
    [n_test, d] over them -- ``est`` and the bounds as odds ratios when ``show_or`` --, NaN where a column was not fitted.
    ``deviance``, ``iterations`` and ``flags`` [n_test] describe the fit (bit 0: not converged within ``maxit``; bit 1:
    rank-deficient or not fittable, the values are NaN; bit 2: a fitted probability numerically 0 or 1); ``lrt_stat`` and
    ``lrt_p`` test the fit against the base model.  ``base`` is the base model: ``name`` (``(Intercept)``, the covariates,
    the conditioned columns), ``est``, ``se``, ``lower``, ``upper``, ``pval`` (never exponentiated), ``deviance``,
    ``iterations``, ``flags``.  ``n_samp`` samples entered, ``n_case`` of them cases; ``n_excluded`` fell to the threshold."""

    def __init__(self, model: str, locus: str, name: List[str], h_names: Tuple[str, ...], est, se, lower, upper, pval, deviance,
                 lrt_stat, lrt_p, iterations, flags, base: Dict[str, object], n_samp: int, n_case: int, n_excluded: int, show_or: bool):
        self.model, self.locus, self.name, self.h_names = model, locus, name, h_names
        self.est, self.se, self.lower, self.upper, self.pval = est, se, lower, upper, pval
        self.deviance, self.lrt_stat, self.lrt_p = deviance, lrt_stat, lrt_p
        self.iterations, self.flags, self.base = iterations, flags, base
        self.n_samp, self.n_case, self.n_excluded, self.show_or = n_samp, n_case, n_excluded, show_or

    def to_table(self) -> Dict[str, np.ndarray]:
        """The columns under the reference's names: per ``h`` column ``h.est``, ``h.2.5%``, ``h.97.5%``, ``h.pval`` (``h1.*``
        then ``h2.*`` for the genotype model), the first three with ``_OR`` appended under ``show_or``; the rows are ``name``."""
        out: Dict[str, np.ndarray] = {}
        sfx = "_OR" if self.show_or else ""
        for j, h in enumerate(self.h_names):
            out[f"{h}.est{sfx}"] = self.est[:, j]
            out[f"{h}.2.5%{sfx}"] = self.lower[:, j]
            out[f"{h}.97.5%{sfx}"] = self.upper[:, j]
            out[f"{h}.pval"] = self.pval[:, j]
        return out

    def __repr__(self):
        return (f"HlaAssocGlmResult({self.model!r}, {len(self.name)} tests, {len(self.base['name']) - 1} covariates, "
                f"{self.n_samp} samples with {self.n_case} cases)")


def _covariates(covariates, n_all: int) -> Tuple[List[str], np.ndarray]:
    """(names, float64 [q, n_all]) from an array [n_all, q] (a vector is one covariate) or a dict name -> vector."""
    if covariates is None:
        return [], np.zeros((0, n_all))
    if isinstance(covariates, dict):
        names = [str(k) for k in covariates]
        cols = [np.asarray(v, np.float64).ravel() for v in covariates.values()]
    else:
        a = np.asarray(covariates, np.float64)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2:
            raise ValueError("'covariates' must be an array [n_samples, q] or a dict of vectors")
        names = [f"c{j + 1}" for j in range(a.shape[1])]
        cols = [a[:, j] for j in range(a.shape[1])]
    for name, c in zip(names, cols):
        if len(c) != n_all:
            raise ValueError(f"covariate {name!r} has {len(c)} values for {n_all} samples")
    return names, (np.stack(cols) if cols else np.zeros((0, n_all)))


def _check_fit_control(maxit, epsilon) -> None:
    if isinstance(maxit, bool) or not isinstance(maxit, (int, np.integer)) or maxit < 1:
        raise ValueError("maxit must be an integer >= 1")
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)) or not epsilon > 0:
        raise ValueError("epsilon must be > 0")


def _design(plan: _Plan, hla: HlaAlleleClass, covariates, use_prob: bool) -> Tuple[List[str], np.ndarray, Optional[np.ndarray]]:
    """(covariate names, covariates [q, n_kept], prior weights [n_kept] or None) over the kept samples of ``plan``."""
    cov_names, cov = _covariates(covariates, len(hla.sample_id))
    cov = np.ascontiguousarray(cov[:, plan.sel])
    if not np.isfinite(cov).all():
        bad = cov_names[int(np.flatnonzero(~np.isfinite(cov).all(axis=1))[0])]
        raise ValueError(f"covariate {bad!r} has a missing or non-finite value: subset the samples first")
    weight = None
    if use_prob:
        if hla.prob is None:
            raise ValueError("No posterior probability in 'hla' ('hla.prob' should be available).")
        weight = np.ascontiguousarray(np.asarray(hla.prob, np.float64)[plan.sel])
        if not (np.isfinite(weight).all() and (weight >= 0).all()):
            raise ValueError("use_prob: the posterior probabilities of the kept samples must be finite and >= 0")
    return cov_names, cov, weight


def _condition_list(condition, what: str = "test") -> List[str]:
    condition = [condition] if isinstance(condition, str) else list(condition) if condition is not None else []
    if any(not isinstance(c, str) for c in condition):
        raise ValueError(f"'condition' is a list of {what} names")
    return condition


def _condition_tests(plan: _Plan, condition: Sequence[str], per: int) -> Tuple[List[int], List[str]]:
    """(device test per name, covariate names of their ``per`` h columns) of ``condition``, names of single tests."""
    rows, names = [], []
    for c in condition:
        if c not in plan.names:
            raise ValueError(f"condition: {c!r} is not a test of this analysis")
        row = plan.row[plan.names.index(c)]
        if row < 0:
            raise ValueError(f"condition: no allele of the data belongs to {c!r}")
        rows.append(row)
        names += [f"h[{c}]"] if per == 1 else [f"h1[{c}]", f"h2[{c}]"]
    return rows, names


def _base_model(coef, se, deviance, iterations, flags, slots: Sequence[int], names: List[str]) -> Dict[str, object]:
    """The ``base`` entry of a result from the base model's fit: its intercept and the covariates in ``slots``."""
    est, sd = coef[list(slots)], se[list(slots)]
    lower, upper, pval = _wald(est, sd)
    return {"name": ["(Intercept)"] + names, "est": est, "se": sd, "lower": lower, "upper": upper, "pval": pval,
            "deviance": float(deviance), "iterations": int(iterations), "flags": int(flags)}


def hlaAssocGlm(hla: HlaAlleleClass, y: Sequence, covariates=None, model: str = "dominant", prob_threshold: float = float("nan"),
                use_prob: bool = False, groups: Optional[HlaAlleleGroups] = None, condition: Optional[Sequence[str]] = None,
                show_or: bool = False, maxit: int = 25, epsilon: float = 1e-8, _backend=None) -> HlaAssocGlmResult:
    """Logistic regression ``y ~ h + covariates`` for every allele of ``hla`` (``hlaAssocTest`` of the reference with a
    formula, ``family = binomial``), on the device.

    * ``hla``, ``y``, ``prob_threshold``, ``groups`` and the list of tests: as ``hlaAssocTest``.
    * ``covariates``: an array [n_samples, q] (columns ``c1``, ``c2``, ...) or a dict name -> vector, float; a non-finite
      value of a kept sample is a ValueError -- no sample is dropped silently.  At most 12 columns with ``condition``.
    * ``model``: the ``h`` column of a test, one value per SAMPLE for every model: ``dominant`` carrier 0 / 1, ``additive``
      the dosage 0 / 1 / 2, ``recessive`` homozygous 0 / 1, ``genotype`` the two dummies ``h1`` (het) and ``h2`` (hom).
    * ``use_prob``: the samples' ``hla.prob`` as prior weights (``weights = prob``); they must be finite and >= 0.
    * ``condition``: names of tests of this analysis whose ``h`` columns join the covariates (both dummies for
      ``genotype``): the stepwise conditional scan.  The conditioned tests themselves come back rank-deficient.
    * ``show_or``: odds ratios -- ``exp`` of the estimates and bounds of the ``h`` columns.
    * ``maxit``, ``epsilon``: ``glm.control``'s.

    A test whose column is constant over the kept samples has flag bit 1 and NaN (R reports NA).  ``genotype``: a dummy that
    nobody carries is left out of the fit (as R's ``as.factor`` drops the level); when nobody is WITHOUT the allele R would
    re-base the factor, which is not mirrored: the test has bit 1.  The likelihood-ratio columns are NaN unless both the fit
    and the base model converged.  A rank-deficient base model is a ValueError.

    Not built: other families (a quantitative trait: ``hlaAssocQuant``), permutation p-values for this
    regression (``hlaAssocScore`` gives the family-wise p-value of the same tests), R's step halving (with the clamps of section 23 the deviance is always finite), interaction terms, and
    ``fisher_p`` of the genotype model.  (``_backend``: the tests' seam -- a class with the interface of ``_DeviceGlm`` that
    stands in for the device.)"""
    _check_model(model)
    _check_fit_control(maxit, epsilon)
    plan = _Plan(hla, y, prob_threshold, groups)
    cov_names, cov, weight = _design(plan, hla, covariates, use_prob)
    condition = _condition_list(condition)
    per = 2 if model == "genotype" else 1
    cond_rows, cond_names = _condition_tests(plan, condition, per)
    cov_names += cond_names
    q = len(cov_names)
    if q > MAX_COVAR:
        raise ValueError(f"{q} covariate columns ({len(condition)} conditioned tests included); at most {MAX_COVAR}")

    backend = _DeviceGlm if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        for row in cond_rows:
            cov = np.concatenate([cov, dev.feature_rows(per * row, per).astype(np.float64)])
        coef, se, dev_t, it, fl = dev.glm(cov, weight, int(maxit), float(epsilon))

    T = plan.n_device_tests
    if fl[T] & FLAG_RANK:
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    d = per
    est, sd, deviance = plan.spread(coef[:T, 1:1 + d]), plan.spread(se[:T, 1:1 + d]), plan.spread(dev_t[:T])
    iterations = plan.spread(it[:T], 0).astype(np.int32)
    flags = plan.spread(fl[:T], FLAG_RANK).astype(np.int32)
    lower, upper, pval = _wald(est, sd)
    bad = ((flags | fl[T]) & (FLAG_MAXIT | FLAG_RANK)) != 0
    lrt_stat = np.where(bad, np.nan, dev_t[T] - deviance)
    df = np.isfinite(est).sum(axis=1)
    with np.errstate(invalid="ignore"):
        chi = np.where(lrt_stat < 0, 0.0, lrt_stat)        # (rounding of two nearly equal deviances)
    lrt_p = np.where(df == 2, _chisq_p(chi, 2), _chisq_p(chi, 1))
    lrt_p[bad | (df == 0)] = np.nan
    if show_or:
        est, lower, upper = np.exp(est), np.exp(lower), np.exp(upper)
    base = _base_model(coef[T], se[T], dev_t[T], it[T], fl[T], [0] + list(range(COV0, COV0 + q)), cov_names)
    return HlaAssocGlmResult(model, hla.locus, plan.names, ("h1", "h2") if d == 2 else ("h",), est, sd, lower, upper, pval, deviance,
                             lrt_stat, lrt_p, iterations, flags, base, plan.n_samp, plan.n_case, plan.n_excluded, bool(show_or))


__all__ = ["HlaAssocGlmResult", "hlaAssocGlm"]
