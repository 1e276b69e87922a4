"""``hlaAssocSurv``: Cox regression per allele for time-to-event traits.

For a follow-up time with a censoring indicator -- graft or patient survival, time to AIDS or to viral rebound, age at onset,
time to a drug reaction -- and covariates ``c1 ... cq``, every test of the analysis (each allele of the typed cohort and, with
``groups``, each level of every partition of the alleles) is one ``coxph(Surv(time, event) ~ h + c1 + ... + cq)``: an estimate
(log hazard ratio, or hazard ratio with ``show_hr``), its confidence interval and Wald p-value per ``h`` column, a
likelihood-ratio test against the base model ``Surv ~ c1 + ... + cq`` and the score test at the base model (the log-rank
test when there are no covariates and no ties).  ``condition`` repeats the scan conditioned on earlier hits.  All fits share
the samples, their order in time and the covariates; they run on the device (``hibag_hip_assoc_cox``), one workgroup per fit:
scans along the risk sets and two 16 x 16 FP64 matrix-core Grams per Newton iteration.  The definitions are DESIGN.md
section 31.

Not built: ``use_prob`` / case weights, strata, left truncation and time-varying covariates, robust variance, step halving
and Firth's correction for monotone likelihoods, permutation or multiplier family-wise p-values, the omnibus and interaction
forms, haplotype dosages as regressors."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _check_model, _Plan, _chisq_p, _is_na, _ptr
from .assocglm import _DeviceGlm, _check_fit_control, _condition_list, _condition_tests, _covariates, _wald
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

MAX_COVAR = 12                     # HIBAG_HIP_COX_MAX_COVAR
SLOTS = 16                         # coefficient slots of a fit: 0 h (het), 1 hom, 2 .. the covariates
COV0 = 2
FLAG_MAXIT, FLAG_RANK, FLAG_CLAMP, FLAG_DECREASE = 1, 2, 4, 8
TIES = ("efron", "breslow")


class _DeviceSurv(_DeviceGlm):
    """The tests of one cohort in time order on the device, with the Cox entry."""

    def cox(self, time: np.ndarray, covar: Optional[np.ndarray], ties: int, maxit: int, epsilon: float):
        """(coef, se [1 + n_tests, 16], loglik, score, iterations, flags [1 + n_tests]), the base model first; time
        [n_kept] not increasing, covar [q, n_kept] centred."""
        n_fit = self.n_tests + 1
        time = np.ascontiguousarray(time, np.float64)
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        coef, se = np.empty((n_fit, SLOTS)), np.empty((n_fit, SLOTS))
        ll, sc, it, fl = np.empty(n_fit), np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_cox(self._h, _ptr(time), _ptr(covar), 0 if covar is None else covar.shape[0], ties, maxit,
                                                  epsilon, None, _ptr(coef), _ptr(se), _ptr(ll), _ptr(sc), _ptr(it), _ptr(fl)))
        return coef, se, ll, sc, it, fl


class HlaAssocSurvResult:
    """The table of ``hlaAssocSurv``, one entry per test in the order of ``hlaAssocTest``.  ``h_names`` are the ``h`` columns,
    ``("h",)`` or, for the genotype model, ``("h1", "h2")`` (het, hom); ``est``, ``se``, ``lower``, ``upper``, ``pval`` are
    [n_test, d] over them -- ``est`` and the bounds as hazard ratios when ``show_hr`` --, NaN where a column was not fitted;
    ``carriers`` and ``carrier_events`` int64 [n_test, d] count the samples with a non-zero ``h`` column and the events among
    them; ``n`` and ``events`` [n_test] the samples and events of the fit (the same for every test).  ``loglik``,
    ``iterations`` and ``flags`` [n_test] describe the fit (bit 0: not converged within ``maxit``; bit 1: a failing pivot, a
    column that cannot be fitted or no event, the values are NaN; bit 2: a linear predictor was clamped to [-200, 200]; bit
    3: the log-likelihood decreased in an iteration that did not converge); ``lrt_stat`` and ``lrt_p`` test the fit against the base model,
    ``score_stat`` and ``score_p`` are the score test at the base model.  ``base`` is the base model: ``name`` (the
    covariates, the conditioned columns), ``est``, ``se``, ``lower``, ``upper``, ``pval`` (never exponentiated), ``loglik``,
    ``iterations``, ``flags``.  ``n_samp`` samples entered, ``n_event`` of them events; ``n_excluded`` fell to the threshold."""

    def __init__(self, model: str, ties: str, locus: str, name: List[str], h_names: Tuple[str, ...], n, events, carriers, carrier_events,
                 est, se, lower, upper, pval, lrt_stat, lrt_p, score_stat, score_p, loglik, iterations, flags, base: Dict[str, object],
                 n_samp: int, n_event: int, n_excluded: int, show_hr: bool):
        self.model, self.ties, self.locus, self.name, self.h_names = model, ties, locus, name, h_names
        self.n, self.events, self.carriers, self.carrier_events = n, events, carriers, carrier_events
        self.est, self.se, self.lower, self.upper, self.pval = est, se, lower, upper, pval
        self.lrt_stat, self.lrt_p, self.score_stat, self.score_p = lrt_stat, lrt_p, score_stat, score_p
        self.loglik, self.iterations, self.flags, self.base = loglik, iterations, flags, base
        self.n_samp, self.n_event, self.n_excluded, self.show_hr = n_samp, n_event, n_excluded, show_hr

    def to_table(self) -> Dict[str, np.ndarray]:
        """The columns: ``n``, ``events``; per ``h`` column ``carriers``, ``carrier_events``, ``h.est``, ``h.se``, ``h.2.5%``,
        ``h.97.5%``, ``h.pval`` (for the genotype model ``h1.carriers`` ... then ``h2.carriers`` ...), the estimate and the
        bounds with ``_HR`` appended under ``show_hr``; ``lrt_stat``, ``lrt_p``, ``score_stat``, ``score_p``, ``loglik``,
        ``iterations``, ``flags``; the rows are ``name``."""
        out: Dict[str, np.ndarray] = {"n": self.n, "events": self.events}
        sfx = "_HR" if self.show_hr else ""
        single = len(self.h_names) == 1
        for j, h in enumerate(self.h_names):
            out["carriers" if single else f"{h}.carriers"] = self.carriers[:, j]
            out["carrier_events" if single else f"{h}.carrier_events"] = self.carrier_events[:, j]
            out[f"{h}.est{sfx}"] = self.est[:, j]
            out[f"{h}.se"] = self.se[:, j]
            out[f"{h}.2.5%{sfx}"] = self.lower[:, j]
            out[f"{h}.97.5%{sfx}"] = self.upper[:, j]
            out[f"{h}.pval"] = self.pval[:, j]
        for key in ("lrt_stat", "lrt_p", "score_stat", "score_p", "loglik", "iterations", "flags"):
            out[key] = getattr(self, key)
        return out

    def __repr__(self):
        return (f"HlaAssocSurvResult({self.model!r}, {self.ties!r}, {len(self.name)} tests, {len(self.base['name'])} covariates, "
                f"{self.n_samp} samples with {self.n_event} events)")


def _time_event(time, event, sel: np.ndarray, n_all: int) -> Tuple[np.ndarray, np.ndarray]:
    """(time float64, event int32) over the kept samples ``sel``: times finite and >= 0, events 0 / 1 or bool."""
    time = list(np.asarray(time, dtype=object).ravel())
    event = list(np.asarray(event, dtype=object).ravel())
    if len(time) != n_all or len(event) != n_all:
        raise ValueError(f"'hla', 'time' and 'event' must have the same length ({n_all} samples, {len(time)} times, {len(event)} events)")
    t, e = np.empty(len(sel)), np.empty(len(sel), np.int32)
    for k, i in enumerate(sel):
        v, ev = time[i], event[i]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"time[{i}] = {v!r}: the times of the kept samples must be finite and >= 0; subset the samples first")
        if _is_na(ev) or not isinstance(ev, (bool, np.bool_, int, float, np.integer, np.floating)) or ev not in (0, 1):
            raise ValueError(f"event[{i}] = {ev!r}: the events of the kept samples must be 0 / 1 or bool; subset the samples first")
        t[k], e[k] = float(v), int(ev)
    return t, e


def hlaAssocSurv(hla: HlaAlleleClass, time: Sequence, event: Sequence, covariates=None, model: str = "dominant",
                 prob_threshold: float = float("nan"), groups: Optional[HlaAlleleGroups] = None, condition: Optional[Sequence[str]] = None,
                 ties: str = "efron", show_hr: bool = False, maxit: int = 20, epsilon: float = 1e-9, _backend=None) -> HlaAssocSurvResult:
    """Cox regression ``Surv(time, event) ~ h + covariates`` for every allele of ``hla``, on the device.

    * ``hla``, ``prob_threshold``, ``groups`` and the list of tests: as ``hlaAssocTest``.  ``model``, ``covariates`` and
      ``condition``: as ``hlaAssocGlm``; the covariates (and the conditioned columns) are centred on their means over the
      kept samples, which leaves the fit where it is and keeps ``exp`` in range.
    * ``time``: one follow-up time per sample, finite and >= 0; ``event``: 1 / True where the event was seen at ``time``,
      0 / False where the sample was censored then.  Anything else in a kept sample is a ValueError -- no sample is dropped
      silently.
    * ``ties``: ``"efron"`` (``coxph``'s default) or ``"breslow"``.
    * ``show_hr``: hazard ratios -- ``exp`` of the estimates and bounds of the ``h`` columns.
    * ``maxit``, ``epsilon``: at most ``maxit`` Newton iterations; converged when the log-likelihood changes by at most
      ``epsilon`` relative.

    A test whose column is constant over the kept samples has flag bit 1 and NaN; the ``genotype`` model drops a dummy that
    nobody carries, as ``hlaAssocGlm``.  With no event among the kept samples every test has bit 1.  A column whose carriers
    (or non-carriers) have no event has a monotone likelihood: it is fitted as it comes and ends with bit 0 and / or bit 2,
    or converged on the flat likelihood with a large estimate and a huge ``se``; its likelihood-ratio and score tests are valid.
    A column whose carriers are the earliest events can lose its information altogether after an overshooting first step
    (their risk dominates every risk set): it has bit 1 and NaN, never a runaway estimate.  A rank-deficient base model is a
    ValueError.  The likelihood-ratio
    columns are NaN only where the fit or the base model has bit 1.

    Not built: ``use_prob`` / case weights, strata, left truncation and time-varying covariates, robust variance, step
    halving and Firth's correction, family-wise p-values, the omnibus and interaction forms, haplotype dosages.
    (``_backend``: the tests' seam -- a class with the interface of ``_DeviceSurv`` that stands in for the device.)"""
    _check_model(model)
    _check_fit_control(maxit, epsilon)
    if ties not in TIES:
        raise ValueError("'ties' should be one of " + ", ".join(f'"{t}"' for t in TIES))
    plan = _Plan(hla, None, prob_threshold, groups)
    n_all = len(hla.sample_id)
    t_kept, e_kept = _time_event(time, event, plan.sel, n_all)
    order = np.argsort(-t_kept, kind="stable")                 # time descending, stable
    plan.sel, plan.a1, plan.a2 = plan.sel[order], np.ascontiguousarray(plan.a1[order]), np.ascontiguousarray(plan.a2[order])
    t_kept, plan.y = np.ascontiguousarray(t_kept[order]), np.ascontiguousarray(e_kept[order])
    plan.n_case = int(plan.y.sum())

    cov_names, cov = _covariates(covariates, n_all)
    cov = np.ascontiguousarray(cov[:, plan.sel])
    if not np.isfinite(cov).all():
        bad = cov_names[int(np.flatnonzero(~np.isfinite(cov).all(axis=1))[0])]
        raise ValueError(f"covariate {bad!r} has a missing or non-finite value: subset the samples first")
    condition = _condition_list(condition)
    per = 2 if model == "genotype" else 1
    cond_rows, cond_names = _condition_tests(plan, condition, per)
    cov_names = cov_names + cond_names
    q = len(cov_names)
    if q > MAX_COVAR:
        raise ValueError(f"{q} covariate columns ({len(condition)} conditioned tests included); at most {MAX_COVAR}")

    backend = _DeviceSurv if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        T = plan.n_device_tests
        feat = dev.feature_rows(0, per * T)
        for row in cond_rows:
            cov = np.concatenate([cov, feat[per * row:per * row + per].astype(np.float64)])
        cov = cov - cov.mean(axis=1, keepdims=True) if q else cov
        coef, se, ll, sc, it, fl = dev.cox(t_kept, cov, TIES.index(ties), int(maxit), float(epsilon))

    if fl[0] & FLAG_RANK and plan.n_case > 0:
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    d = per
    carried = (feat != 0).astype(np.int64)
    carriers = plan.spread(carried.sum(axis=1).reshape(T, d), 0).astype(np.int64)
    carrier_events = plan.spread((carried @ plan.y.astype(np.int64)).reshape(T, d), 0).astype(np.int64)
    est, sd, loglik = plan.spread(coef[1:, :d]), plan.spread(se[1:, :d]), plan.spread(ll[1:])
    score_stat = plan.spread(sc[1:])
    iterations = plan.spread(it[1:], 0).astype(np.int32)
    flags = plan.spread(fl[1:], FLAG_RANK).astype(np.int32)
    lower, upper, pval = _wald(est, sd)
    bad = ((flags | fl[0]) & FLAG_RANK) != 0
    with np.errstate(invalid="ignore"):
        lrt_stat = np.where(bad, np.nan, 2.0 * (loglik - ll[0]))
        chi = np.where(lrt_stat < 0, 0.0, lrt_stat)            # (rounding of two nearly equal log-likelihoods)
    df = np.isfinite(est).sum(axis=1)
    lrt_p = np.where(df == 2, _chisq_p(chi, 2), _chisq_p(chi, 1))
    lrt_p[bad | (df == 0)] = np.nan
    score_p = np.where(df == 2, _chisq_p(score_stat, 2), _chisq_p(score_stat, 1))
    score_p[bad | (df == 0)] = np.nan
    if show_hr:
        est, lower, upper = np.exp(est), np.exp(lower), np.exp(upper)
    b_est, b_se = coef[0, COV0:COV0 + q], se[0, COV0:COV0 + q]
    b_lower, b_upper, b_pval = _wald(b_est, b_se)
    base = {"name": cov_names, "est": b_est, "se": b_se, "lower": b_lower, "upper": b_upper, "pval": b_pval,
            "loglik": float(ll[0]), "iterations": int(it[0]), "flags": int(fl[0])}
    n_test = len(plan.names)
    return HlaAssocSurvResult(model, ties, hla.locus, plan.names, ("h1", "h2") if d == 2 else ("h",),
                              np.full(n_test, plan.n_samp, np.int64), np.full(n_test, plan.n_case, np.int64), carriers, carrier_events,
                              est, sd, lower, upper, pval, lrt_stat, lrt_p, score_stat, score_p, loglik, iterations, flags, base,
                              plan.n_samp, plan.n_case, plan.n_excluded, bool(show_hr))


__all__ = ["HlaAssocSurvResult", "hlaAssocSurv"]
