"""``hlaAssocOmnibus`` and ``hlaAssocStepwise``: the omnibus test of an amino-acid position, and the stepwise conditional scan.

HLA fine-mapping asks of a position -- DRB1 position 11 with all its residues, or the two-digit types, or any partition of
the alleles built by ``hlaGroupsBySequence`` / ``hlaGroupsByResolution`` -- whether it explains a case / control trait beyond
the covariates: the likelihood-ratio test of ``glm(y ~ r_1 + ... + r_d + covariates, family = binomial)`` against
``glm(y ~ covariates, family = binomial)``, d = (carried levels - 1) degrees of freedom, then again conditioned on the
positions already found.  One test per partition of ``groups``; every fit runs on the device
(``hibag_hip_assoc_glm_sets``), one workgroup per fit over a 32-slot design whose 32 x 32 normal matrix is three 16 x 16
FP64 matrix-core blocks per four samples.  Aliased columns are dropped as R's ``glm.fit`` drops them and the degrees of
freedom shrink with them.  The definitions are DESIGN.md section 26 (the fit itself: section 23).

Not built: permutation p-values for these fits (``hlaAssocScore(..., omnibus=True)``, assocscore.py, has the family-wise p-value
of the same design sets), the ``genotype`` coding, lumping of rare levels, designs beyond 31 columns,
interactions, other families."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _check_model, _Plan, _ptr, chisq_sf
from .assocglm import (FLAG_MAXIT, FLAG_RANK, _base_model, _check_fit_control, _condition_list, _condition_tests, _design, _DeviceGlm,
                       _wald)
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

SLOTS = 32                         # HIBAG_HIP_GLM_WIDE_SLOTS: 0 intercept, 1 .. H the set's rows, 1 + H .. H + q the covariates
MAX_COLUMNS = 30                   # a set's rows and the covariates together
MAX_COVAR = 29
FLAG_ALIASED, FLAG_TOO_WIDE = 8, 16
OMNIBUS_MODELS = ("additive", "dominant", "recessive")


class _DeviceOmni(_DeviceGlm):
    """The tests of one cohort on the device, with the set regression."""

    def row_sums(self) -> np.ndarray:
        """int32 [feature rows]: each row's sum over the kept samples."""
        out = np.empty(self.n_rows, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_row_sums(self._h, _ptr(out)))
        return out

    def glm_sets(self, sets: Sequence[Sequence[int]], covar: Optional[np.ndarray], weight: Optional[np.ndarray], maxit: int,
                 epsilon: float):
        """(coef, se [n_sets + 1, 32], deviance, iterations, flags, df_h [n_sets + 1]) of the sets of feature rows and, last,
        the base model; covar [q, n_kept], weight [n_kept]."""
        n_fit = len(sets) + 1
        start = np.zeros(n_fit, np.int32)
        start[1:] = np.cumsum([len(s) for s in sets])
        rows = np.ascontiguousarray([r for s in sets for r in s] or [0], np.int32)
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        weight = None if weight is None else np.ascontiguousarray(weight, np.float64)
        coef, se = np.empty((n_fit, SLOTS)), np.empty((n_fit, SLOTS))
        dev, it, fl, df = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_glm_sets(self._h, _ptr(start), _ptr(rows), len(sets), _ptr(covar),
                                                       0 if covar is None else covar.shape[0], _ptr(weight), maxit, epsilon,
                                                       _ptr(coef), _ptr(se), _ptr(dev), _ptr(it), _ptr(fl), _ptr(df)))
        return coef, se, dev, it, fl, df


class HlaAssocOmnibusResult:
    """The table of ``hlaAssocOmnibus``, one entry per partition of ``groups`` in partition order.

    Per partition: ``name``; ``n_levels``, the levels that a kept sample carries; ``reference``, the name of the level left
    out of the design (the most frequent one; ``None`` where the partition is not tested); ``df``, the columns still in the
    fit at its last solve; ``deviance``; ``lrt_stat`` = the base model's deviance minus the fit's and ``lrt_p``, its
    chi-square tail with ``df`` degrees of freedom (NaN when either fit has flag bit 0 or 1, or ``df`` is 0); ``iterations``;
    ``flags`` (bit 0: not converged within ``maxit``; bit 1: not tested or rank-deficient, the values are NaN; bit 2: a
    fitted probability numerically 0 or 1; bit 3: a column was dropped as aliased; bit 4: more columns than the design holds).

    Per level, lists over the partitions of arrays over ALL levels of the partition in ``groups``' order: ``level_names``,
    ``est`` (log odds ratio against the reference level), ``se``, ``lower``, ``upper``, ``pval`` -- NaN for the reference, for
    dropped columns and for levels that no kept sample carries.

    ``base`` is the base model as ``hlaAssocGlm`` reports it (``name``: ``(Intercept)``, the covariates, the conditioned
    columns; a conditioned column dropped as aliased has NaN).  ``n_samp`` samples entered, ``n_case`` of them cases;
    ``n_excluded`` fell to the threshold."""

    def __init__(self, model: str, locus: str, name: List[str], n_levels, reference: List[Optional[str]], df, deviance, lrt_stat,
                 lrt_p, iterations, flags, level_names: List[List[str]], est, se, lower, upper, pval, base: Dict[str, object],
                 n_samp: int, n_case: int, n_excluded: int):
        self.model, self.locus, self.name, self.n_levels, self.reference = model, locus, name, n_levels, reference
        self.df, self.deviance, self.lrt_stat, self.lrt_p = df, deviance, lrt_stat, lrt_p
        self.iterations, self.flags = iterations, flags
        self.level_names, self.est, self.se, self.lower, self.upper, self.pval = level_names, est, se, lower, upper, pval
        self.base, self.n_samp, self.n_case, self.n_excluded = base, n_samp, n_case, n_excluded

    def to_table(self) -> Dict[str, np.ndarray]:
        """The per-partition columns; the rows are ``name``."""
        return {"n.levels": self.n_levels, "df": self.df, "deviance": self.deviance, "lrt.st": self.lrt_stat, "lrt.p": self.lrt_p}

    def __repr__(self):
        return (f"HlaAssocOmnibusResult({self.model!r}, {len(self.name)} partitions, {len(self.base['name']) - 1} covariate columns, "
                f"{self.n_samp} samples with {self.n_case} cases)")


class HlaAssocStepwiseResult:
    """What ``hlaAssocStepwise`` did: ``steps``, the scan of every round (``HlaAssocOmnibusResult``; round k is conditioned on
    ``chosen[:k]``), ``chosen``, the partitions taken in order, and ``lrt_p``, the p-value each was taken with."""

    def __init__(self, steps: List[HlaAssocOmnibusResult], chosen: List[str], lrt_p: List[float]):
        self.steps, self.chosen, self.lrt_p = steps, chosen, lrt_p

    def __repr__(self):
        return f"HlaAssocStepwiseResult({len(self.steps)} scans, chosen {self.chosen!r})"


def _partition_rows(plan: _Plan, groups: HlaAlleleGroups) -> List[List[int]]:
    """Per partition and level the device's feature row (-1: a level the device does not know), from the plan's test list:
    the alleles come first, then every partition's levels in order."""
    out, at = [], len(plan.alleles)
    for q in range(groups.n_part):
        k = len(groups.levels[q])
        out.append([int(r) for r in plan.row[at:at + k]])
        at += k
    return out


def _design_sets(part_rows: List[List[int]], rsum: np.ndarray) -> Tuple[List[List[int]], List[int], List[int]]:
    """Per partition (the levels in its set, its reference level or -1, its number of carried levels): the carried levels are
    those the device knows with a positive row sum; the reference is the one with the largest row sum, on a tie the lowest
    level; the set is every other carried level in level order -- empty when fewer than two levels are carried."""
    sets, ref, carried_n = [], [], []
    for rows in part_rows:
        carried = [lv for lv, r in enumerate(rows) if r >= 0 and rsum[r] > 0]
        carried_n.append(len(carried))
        if len(carried) < 2:
            sets.append([])
            ref.append(-1)
            continue
        best = max(carried, key=lambda lv: (int(rsum[rows[lv]]), -lv))
        ref.append(best)
        sets.append([lv for lv in carried if lv != best])
    return sets, ref, carried_n


def hlaAssocOmnibus(hla: HlaAlleleClass, y: Sequence, groups: HlaAlleleGroups, covariates=None, model: str = "additive",
                    prob_threshold: float = float("nan"), use_prob: bool = False, condition: Optional[Sequence[str]] = None,
                    maxit: int = 25, epsilon: float = 1e-8, _backend=None) -> HlaAssocOmnibusResult:
    """The omnibus test of every partition of ``groups``: ``y ~ levels + covariates`` against ``y ~ covariates``, logistic, on
    the device.

    * ``hla``, ``y``, ``prob_threshold``, ``covariates``, ``use_prob``, ``maxit``, ``epsilon``: as ``hlaAssocGlm``, except that
      covariates and conditioned columns together may number 29.
    * ``groups``: the partitions (``hlaGroupsBySequence``: one per amino-acid position; ``hlaGroupsByResolution``).  A
      partition's design has one column per level that a kept sample carries, except the reference level -- the level with
      the largest column sum, on a tie the first --, which the intercept absorbs.  A partition with fewer than two carried
      levels is not tested (flag bit 1); one with more than ``30 - covariate columns`` columns is not either (bits 4 and 1).
    * ``model``: a level's column per sample: ``additive`` the number of the sample's alleles in the level (the default),
      ``dominant`` 0 / 1 carrier, ``recessive`` 0 / 1 both alleles.  ``genotype`` is not built: ValueError.
    * ``condition``: names of partitions -- all non-reference columns of each join the covariates -- or of single tests as
      ``hlaAssocGlm`` takes them (an allele, or ``partition:level``).  A conditioned partition itself comes back with every
      column dropped: ``df`` 0, ``lrt_p`` NaN.

    A column that is a linear combination of the intercept, the covariates and the columns before it is dropped, as R's
    ``glm.fit`` drops it: NaN in its place, flag bit 3, one degree of freedom less.  A base model that is rank-deficient in
    the user's covariates is a ValueError; a conditioned column that is aliased there is dropped and reported NaN in ``base``.
    (``_backend``: the tests' seam -- a class with the interface of ``_DeviceOmni`` that stands in for the device.)"""
    if model == "genotype":
        raise ValueError("the genotype coding is not built for the omnibus test: additive, dominant or recessive")
    _check_model(model, OMNIBUS_MODELS)
    if not isinstance(groups, HlaAlleleGroups):
        raise TypeError("'groups' must be an HlaAlleleGroups")
    _check_fit_control(maxit, epsilon)
    plan = _Plan(hla, y, prob_threshold, groups)
    cov_names, cov, weight = _design(plan, hla, covariates, use_prob)
    n_user = len(cov_names)
    condition = _condition_list(condition, "partition or test")
    part_names = list(groups.names)
    part_rows = _partition_rows(plan, groups)
    for c in condition:
        if c not in part_names and c not in plan.names:
            raise ValueError(f"condition: {c!r} is neither a partition nor a test of this analysis")

    backend = _DeviceOmni if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        sets, ref, carried_n = _design_sets(part_rows, dev.row_sums())
        cond_rows: List[int] = []
        for c in condition:
            if c in part_names:
                p = part_names.index(c)
                if not sets[p]:
                    raise ValueError(f"condition: partition {c!r} has fewer than two levels among the kept samples")
                cond_rows += [part_rows[p][lv] for lv in sets[p]]
                cov_names += [f"h[{c}:{groups.levels[p][lv]}]" for lv in sets[p]]
            else:
                rows, names = _condition_tests(plan, [c], 1)
                cond_rows += rows
                cov_names += names
        q = len(cov_names)
        if q > MAX_COVAR:
            raise ValueError(f"{q} covariate columns ({q - n_user} conditioned columns included); at most {MAX_COVAR}")
        for row in cond_rows:
            cov = np.concatenate([cov, dev.feature_rows(row, 1).astype(np.float64)])
        row_sets = [[part_rows[p][lv] for lv in s] for p, s in enumerate(sets)]
        coef, se, dev_t, it, fl, dfh = dev.glm_sets(row_sets, cov, weight, int(maxit), float(epsilon))

    P = len(sets)
    H = max([len(s) for s in sets if 0 < len(s) <= MAX_COLUMNS - q], default=0)
    cov_slots = list(range(1 + H, 1 + H + q))
    # H restates the entry's rule for which sets are fitted; the base model's NaN pattern says where the entry put the
    # covariates (its h slots and everything past the covariates are NaN, the intercept is not unless the fit failed)
    if not (np.isnan(coef[P, 1:1 + H]).all() and np.isnan(coef[P, 1 + H + q:]).all() and
            (fl[P] & FLAG_RANK or (np.isfinite(coef[P, 0]) and (fl[P] & FLAG_ALIASED or np.isfinite(coef[P, cov_slots]).all())))):
        raise RuntimeError("hlaAssocOmnibus: the slot layout of hibag_hip_assoc_glm_sets is not the one expected")
    if fl[P] & FLAG_RANK or np.isnan(coef[P, cov_slots[:n_user]]).any():
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    bad = ((fl[:P] | fl[P]) & (FLAG_MAXIT | FLAG_RANK)) != 0
    deviance = np.array(dev_t[:P], np.float64)
    lrt_stat = np.where(bad, np.nan, dev_t[P] - deviance)
    df = np.array(dfh[:P], np.int32)
    lrt_p = np.array([math.nan if bad[p] or df[p] == 0 else chisq_sf(float(lrt_stat[p]), int(df[p])) for p in range(P)])
    level_names, est, sd = [], [], []
    for p, s in enumerate(sets):
        k = len(part_rows[p])
        e, d = np.full(k, np.nan), np.full(k, np.nan)
        if s:
            e[s], d[s] = coef[p, 1:1 + len(s)], se[p, 1:1 + len(s)]
        level_names.append(list(groups.levels[p]))
        est.append(e)
        sd.append(d)
    wald = [_wald(e, d) for e, d in zip(est, sd)]
    base = _base_model(coef[P], se[P], dev_t[P], it[P], fl[P], [0] + cov_slots, cov_names)
    reference = [None if r < 0 else groups.levels[p][r] for p, r in enumerate(ref)]
    return HlaAssocOmnibusResult(model, hla.locus, part_names, np.array(carried_n, np.int32), reference, df, deviance, lrt_stat, lrt_p,
                                 np.array(it[:P], np.int32), np.array(fl[:P], np.int32), level_names, est, sd,
                                 [w[0] for w in wald], [w[1] for w in wald], [w[2] for w in wald], base, plan.n_samp, plan.n_case,
                                 plan.n_excluded)


def hlaAssocStepwise(hla: HlaAlleleClass, y: Sequence, groups: HlaAlleleGroups, covariates=None, model: str = "additive",
                     prob_threshold: float = float("nan"), use_prob: bool = False, condition: Optional[Sequence[str]] = None,
                     maxit: int = 25, epsilon: float = 1e-8, p_stop: float = 5e-8, max_steps: int = 10,
                     _backend=None) -> HlaAssocStepwiseResult:
    """The stepwise conditional scan: ``hlaAssocOmnibus``, then again conditioned on the partition with the smallest ``lrt_p``
    (ties: the larger ``lrt_stat``, then partition order), until the smallest ``lrt_p`` is above ``p_stop``, ``max_steps``
    partitions are chosen, or the chosen partition's columns no longer fit among the 29 covariate columns.  ``condition``
    names what every round is conditioned on from the start.  The other arguments are ``hlaAssocOmnibus``'s."""
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 0:
        raise ValueError("max_steps must be an integer >= 0")
    if isinstance(p_stop, bool) or not isinstance(p_stop, (int, float, np.integer, np.floating)) or not 0 <= p_stop <= 1:
        raise ValueError("p_stop must be in [0, 1]")
    cond = [condition] if isinstance(condition, str) else list(condition) if condition is not None else []
    steps: List[HlaAssocOmnibusResult] = []
    chosen: List[str] = []
    taken_p: List[float] = []
    while True:
        res = hlaAssocOmnibus(hla, y, groups, covariates, model, prob_threshold, use_prob, cond + chosen, maxit, epsilon, _backend)
        steps.append(res)
        if len(chosen) >= max_steps:
            break
        order = sorted((p for p in range(len(res.name)) if not math.isnan(res.lrt_p[p])),
                       key=lambda p: (res.lrt_p[p], -res.lrt_stat[p], p))
        if not order or res.lrt_p[order[0]] > p_stop:
            break
        best = order[0]
        if len(res.base["name"]) - 1 + int(res.n_levels[best]) - 1 > MAX_COVAR:        # the column budget
            break
        chosen.append(res.name[best])
        taken_p.append(float(res.lrt_p[best]))
    return HlaAssocStepwiseResult(steps, chosen, taken_p)


__all__ = ["HlaAssocOmnibusResult", "HlaAssocStepwiseResult", "hlaAssocOmnibus", "hlaAssocStepwise"]
