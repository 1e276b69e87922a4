"""``hlaAssocInteract``: the pairwise allele interaction scan.

Fine-mapping asks it straight after the stepwise scan: does the risk of carrying the alleles *a* and *b* together differ
from the product of their separate risks (Lenz et al. 2015, non-additive and interaction effects within HLA loci)?  Per
pair two logistic regressions -- ``y ~ a + b + covariates`` and ``y ~ a + b + a:b + covariates`` -- and the likelihood-ratio
test between them on one degree of freedom; for two alleles of one locus the product column ``a:b`` is the a/b
heterozygote indicator.  All fits of a scan are ONE device call (``hibag_hip_assoc_glm_terms``), one workgroup per fit: the
product column is formed from the two int8 feature rows while the samples are walked and is never written to memory; which
pairs are carried together comes from the int8 Gram of the feature rows (``hibag_hip_assoc_row_gram``), exact.  The fit is
``hlaAssocGlm``'s with the aliased-column rule of ``hlaAssocOmnibus``.  The definitions are DESIGN.md section 27.

Not built: products of more than two rows, position x position omnibus interactions ((L_a - 1)(L_b - 1) product columns),
allele x covariate interactions, a partner matrix from another locus, permutation p-values, the ``genotype`` coding."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _check_model, _Plan, _ptr, chisq_sf
from .assocglm import FLAG_MAXIT, FLAG_RANK, _base_model, _check_fit_control, _condition_list, _condition_tests, _design, _wald
from .assocomni import FLAG_ALIASED, _DeviceOmni  # noqa: F401  (the flag bit 3 of the results)
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

SLOTS = 16                         # 0 intercept, 1 .. 3 the terms, 4 .. 3 + q the covariates
TERMS = 3
COV0 = 4                           # GLMT_COV0
MAX_COVAR = 11                     # HIBAG_HIP_GLM_TERMS_MAX_COVAR
MAX_GRAM_ROWS = 8192               # rows of one hibag_hip_assoc_row_gram call
INTERACT_MODELS = ("additive", "dominant", "recessive")
TERM_NAMES = ("a", "b", "a:b")


class _DeviceInteract(_DeviceOmni):
    """The tests of one cohort on the device, with the term regression."""

    def row_gram(self, row0: int, n_rows: int) -> np.ndarray:
        """int32 [n_rows, n_rows]: the sums over the kept samples of the products of feature rows row0 .. row0 + n_rows - 1."""
        out = np.empty((n_rows, n_rows), np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_row_gram(self._h, row0, n_rows, _ptr(out)))
        return out

    def glm_terms(self, terms: np.ndarray, covar: Optional[np.ndarray], weight: Optional[np.ndarray], maxit: int, epsilon: float):
        """(coef, se [n_fits + 1, 16], deviance, iterations, flags, df_h [n_fits + 1]) of the fit records terms
        [n_fits, 3, 2] and, last, the base model; covar [q, n_kept], weight [n_kept]."""
        terms = np.ascontiguousarray(terms, np.int32).reshape(-1, TERMS, 2)
        n_fit = len(terms) + 1
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        weight = None if weight is None else np.ascontiguousarray(weight, np.float64)
        coef, se = np.empty((n_fit, SLOTS)), np.empty((n_fit, SLOTS))
        dev, it, fl, df = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_glm_terms(self._h, _ptr(terms) if len(terms) else None, len(terms), _ptr(covar),
                                                        0 if covar is None else covar.shape[0], _ptr(weight), maxit, epsilon,
                                                        _ptr(coef), _ptr(se), _ptr(dev), _ptr(it), _ptr(fl), _ptr(df)))
        return coef, se, dev, it, fl, df


class HlaAssocInteractResult:
    """The table of ``hlaAssocInteract``, one entry per pair in the order scanned.

    Per pair: ``name_a``, ``name_b``; ``both``, the sum over the kept samples of the product column (who carries the two
    together); ``est``, ``se``, ``lower``, ``upper``, ``pval`` [n_pair, 3] over ``term_names`` = (``a``, ``b``, ``a:b``), the
    columns of the FULL fit ``y ~ a + b + a:b + covariates`` -- ``est`` and the bounds as odds ratios when ``show_or`` --, NaN
    for a column that was dropped as aliased or left out; ``deviance_main`` (``y ~ a + b + covariates``), ``deviance_full``,
    ``lrt_stat`` = their difference and ``lrt_p``, its chi-square tail on one degree of freedom -- NaN when either fit has flag
    bit 0 or 1, or when the product is not in the full fit at its last solve (``df_full - df_main`` is not 1); ``df_main``,
    ``df_full``, ``flags_main``, ``flags_full``, ``iterations_main``, ``iterations_full`` (the bits: 0 not converged within
    ``maxit``; 1 not fitted or rank-deficient, the values are NaN; 2 a fitted probability numerically 0 or 1; 3 a column was
    dropped as aliased).  A pair with ``both < min_both`` is not fitted: bit 1 and NaN.

    ``base`` is the base model as ``hlaAssocGlm`` reports it.  ``n_samp`` samples entered, ``n_case`` of them cases;
    ``n_excluded`` fell to the threshold."""

    term_names = TERM_NAMES

    def __init__(self, model: str, locus: str, name_a: List[str], name_b: List[str], both, est, se, lower, upper, pval, deviance_main,
                 deviance_full, lrt_stat, lrt_p, df_main, df_full, flags_main, flags_full, iterations_main, iterations_full,
                 base: Dict[str, object], n_samp: int, n_case: int, n_excluded: int, show_or: bool):
        self.model, self.locus, self.name_a, self.name_b, self.both = model, locus, name_a, name_b, both
        self.est, self.se, self.lower, self.upper, self.pval = est, se, lower, upper, pval
        self.deviance_main, self.deviance_full, self.lrt_stat, self.lrt_p = deviance_main, deviance_full, lrt_stat, lrt_p
        self.df_main, self.df_full, self.flags_main, self.flags_full = df_main, df_full, flags_main, flags_full
        self.iterations_main, self.iterations_full = iterations_main, iterations_full
        self.base, self.n_samp, self.n_case, self.n_excluded, self.show_or = base, n_samp, n_case, n_excluded, show_or

    def to_table(self) -> Dict[str, np.ndarray]:
        """``both``, per column of the full fit ``<term>.est``, ``<term>.2.5%``, ``<term>.97.5%`` (with ``_OR`` appended under
        ``show_or``) and ``<term>.pval``, then ``lrt.st`` and ``lrt.p``; the rows are the pairs (``name_a``, ``name_b``)."""
        out: Dict[str, np.ndarray] = {"both": self.both}
        sfx = "_OR" if self.show_or else ""
        for j, t in enumerate(self.term_names):
            out[f"{t}.est{sfx}"] = self.est[:, j]
            out[f"{t}.2.5%{sfx}"] = self.lower[:, j]
            out[f"{t}.97.5%{sfx}"] = self.upper[:, j]
            out[f"{t}.pval"] = self.pval[:, j]
        out["lrt.st"], out["lrt.p"] = self.lrt_stat, self.lrt_p
        return out

    def __repr__(self):
        return (f"HlaAssocInteractResult({self.model!r}, {len(self.name_a)} pairs, {len(self.base['name']) - 1} covariates, "
                f"{self.n_samp} samples with {self.n_case} cases)")


def _pair_rows(plan: _Plan, pairs, rsum: np.ndarray) -> Tuple[List[Tuple[int, int]], List[str], List[str]]:
    """(feature rows, names a, names b) of the pairs to scan: every unordered pair of allele tests with a positive row sum in
    test order (a before b), or exactly ``pairs``."""
    if pairs is None:
        carried = [t for t in range(len(plan.alleles)) if rsum[plan.row[t]] > 0]
        tests = [(a, b) for i, a in enumerate(carried) for b in carried[i + 1:]]
        return [(plan.row[a], plan.row[b]) for a, b in tests], [plan.names[a] for a, _ in tests], [plan.names[b] for _, b in tests]
    rows, name_a, name_b = [], [], []
    for pr in list(pairs):
        if isinstance(pr, str) or len(pr) != 2 or any(not isinstance(c, str) for c in pr):
            raise ValueError("'pairs' is a list of (name, name)")
        for c in pr:
            if c not in plan.names:
                raise ValueError(f"pairs: {c!r} is not a test of this analysis")
            if plan.row[plan.names.index(c)] < 0:
                raise ValueError(f"pairs: no allele of the data belongs to {c!r}")
        a, b = (plan.row[plan.names.index(c)] for c in pr)
        if a == b:
            raise ValueError(f"pairs: {pr[0]!r} is paired with itself")
        rows.append((a, b))
        name_a.append(pr[0])
        name_b.append(pr[1])
    return rows, name_a, name_b


def _both(dev, rows: List[Tuple[int, int]]) -> np.ndarray:
    """int64 [n_pair]: the sum of the product column of every pair, from the Gram of the feature rows between the lowest and
    the highest row named (rows further apart than one Gram call holds: from the two rows themselves; integers either way)."""
    if not rows:
        return np.zeros(0, np.int64)
    lo, hi = min(min(r) for r in rows), max(max(r) for r in rows)
    if hi - lo + 1 <= MAX_GRAM_ROWS:
        G = dev.row_gram(lo, hi - lo + 1)
        return np.array([G[a - lo, b - lo] for a, b in rows], np.int64)
    return np.array([int(dev.feature_rows(a, 1)[0].astype(np.int64) @ dev.feature_rows(b, 1)[0].astype(np.int64)) for a, b in rows],
                    np.int64)


def hlaAssocInteract(hla: HlaAlleleClass, y: Sequence, covariates=None, model: str = "additive", prob_threshold: float = float("nan"),
                     use_prob: bool = False, groups: Optional[HlaAlleleGroups] = None, pairs: Optional[Sequence[Tuple[str, str]]] = None,
                     condition: Optional[Sequence[str]] = None, min_both: int = 1, maxit: int = 25, epsilon: float = 1e-8,
                     show_or: bool = False, _backend=None) -> HlaAssocInteractResult:
    """The interaction scan over pairs of tests: ``y ~ a + b + a:b + covariates`` against ``y ~ a + b + covariates``, logistic,
    on the device.

    * ``hla``, ``y``, ``prob_threshold``, ``covariates``, ``use_prob``, ``groups`` and the list of tests, ``condition``,
      ``show_or``, ``maxit``, ``epsilon``: as ``hlaAssocGlm``, except that covariates and conditioned columns together may
      number 11.
    * ``model``: a test's column per sample: ``additive`` the dosage 0 / 1 / 2 (the default), ``dominant`` carrier 0 / 1,
      ``recessive`` homozygous 0 / 1; the product column is the product of the two columns.  ``genotype`` is a ValueError.
    * ``pairs``: ``None`` scans every unordered pair of ALLELE tests with a positive column sum, in test order; a list of
      ``(name, name)`` scans exactly those pairs -- the names are those ``condition`` takes, the levels of ``groups``'
      partitions (``partition:level``) included.  An unknown name, or a test paired with itself, is a ValueError.
    * ``min_both``: a pair whose product column sums to less than this over the kept samples is not fitted (flag bit 1, NaN).

    A column that is a linear combination of the intercept, the covariates and the columns before it (the order: ``a``,
    ``b``, ``a:b``) is dropped as R's ``glm.fit`` drops it: NaN in its place and flag bit 3; without the product in the full
    fit there is no test and ``lrt_p`` is NaN.  A base model that is rank-deficient in the user's covariates is a ValueError.
    (``_backend``: the tests' seam -- a class with the interface of ``_DeviceInteract`` that stands in for the device.)"""
    if model == "genotype":
        raise ValueError("the genotype coding is not built for the interaction scan: additive, dominant or recessive")
    _check_model(model, INTERACT_MODELS)
    _check_fit_control(maxit, epsilon)
    if isinstance(min_both, bool) or not isinstance(min_both, (int, np.integer)) or min_both < 0:
        raise ValueError("min_both must be an integer >= 0")
    plan = _Plan(hla, y, prob_threshold, groups)
    cov_names, cov, weight = _design(plan, hla, covariates, use_prob)
    n_user = len(cov_names)
    condition = _condition_list(condition)
    cond_rows, cond_names = _condition_tests(plan, condition, 1)
    cov_names += cond_names
    q = len(cov_names)
    if q > MAX_COVAR:
        raise ValueError(f"{q} covariate columns ({len(condition)} conditioned tests included); at most {MAX_COVAR}")

    backend = _DeviceInteract if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        rows, name_a, name_b = _pair_rows(plan, pairs, dev.row_sums())
        both = _both(dev, rows)
        for row in cond_rows:
            cov = np.concatenate([cov, dev.feature_rows(row, 1).astype(np.float64)])
        sub = np.flatnonzero(both >= min_both)
        terms = np.full((2 * len(sub), TERMS, 2), -1, np.int32)
        for i, p in enumerate(sub):
            a, b = rows[p]
            terms[2 * i, 0, 0] = terms[2 * i + 1, 0, 0] = a
            terms[2 * i, 1, 0] = terms[2 * i + 1, 1, 0] = b
            terms[2 * i + 1, 2] = (a, b)
        coef, se, dev_t, it, fl, dfh = dev.glm_terms(terms, cov, weight, int(maxit), float(epsilon))

    B = 2 * len(sub)
    cov_slots = list(range(COV0, COV0 + q))
    if fl[B] & FLAG_RANK or np.isnan(coef[B, cov_slots[:n_user]]).any():
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    P = len(rows)
    est, sd = np.full((P, TERMS), np.nan), np.full((P, TERMS), np.nan)
    dev_main, dev_full = np.full(P, np.nan), np.full(P, np.nan)
    fl_main, fl_full = np.full(P, FLAG_RANK, np.int32), np.full(P, FLAG_RANK, np.int32)
    it_main, it_full, df_main, df_full = (np.zeros(P, np.int32) for _ in range(4))
    est[sub], sd[sub] = coef[1:B:2, 1:1 + TERMS], se[1:B:2, 1:1 + TERMS]
    dev_main[sub], dev_full[sub] = dev_t[0:B:2], dev_t[1:B:2]
    fl_main[sub], fl_full[sub], it_main[sub], it_full[sub] = fl[0:B:2], fl[1:B:2], it[0:B:2], it[1:B:2]
    df_main[sub], df_full[sub] = dfh[0:B:2], dfh[1:B:2]
    lower, upper, pval = _wald(est, sd)
    bad = (((fl_main | fl_full) & (FLAG_MAXIT | FLAG_RANK)) != 0) | (df_full - df_main != 1)
    lrt_stat = np.where(((fl_main | fl_full) & (FLAG_MAXIT | FLAG_RANK)) != 0, np.nan, dev_main - dev_full)
    lrt_p = np.array([math.nan if bad[p] else chisq_sf(float(lrt_stat[p]), 1) for p in range(P)])
    if show_or:
        est, lower, upper = np.exp(est), np.exp(lower), np.exp(upper)
    base = _base_model(coef[B], se[B], dev_t[B], it[B], fl[B], [0] + cov_slots, cov_names)
    return HlaAssocInteractResult(model, hla.locus, name_a, name_b, both, est, sd, lower, upper, pval, dev_main, dev_full, lrt_stat, lrt_p,
                                  df_main, df_full, fl_main, fl_full, it_main, it_full, base, plan.n_samp, plan.n_case,
                                  plan.n_excluded, bool(show_or))


__all__ = ["HlaAssocInteractResult", "hlaAssocInteract"]
