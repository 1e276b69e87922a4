"""``hlaAssocScore``: covariate-adjusted score tests of a case / control trait, with family-wise p-values by multiplier
resampling.

The analysis a case / control study of HLA runs is logistic regression adjusted for sex, age and ancestry components, per
allele and per amino-acid position -- hundreds of correlated tests, whose family-wise p-value Bonferroni overstates.  Under
the base model ``glm(y ~ covariates, family = binomial)``, fitted once, every test's score statistic is a quadratic form in
``U = X~'(y - mu)``, chi-square with one degree of freedom per column; Lin's multiplier resampling (Bioinformatics 21:781,
2005) replaces every sample's residual ``e_i`` by ``e_i s_i`` with independent signs, which keeps each sample's own variance
-- what a permutation of a binary trait under covariates does not -- and repeats no fit.  All tests under all replicates are
one real-valued Gram matrix, int8 feature rows x FP64 resampled residuals, on the FP64 matrix cores
(``hibag_hip_assoc_score_*``).  ``perm_p`` is the pointwise and ``perm_p_adj`` the family-wise p-value (single-step min-P over
the tests, exact through the per-replicate maxima per degree of freedom).  The result is defined exactly
and does not depend on panel sizes or on how the replicates are split over calls.

Not built: product columns (``hlaAssocInteract``), Gaussian multipliers, resampling under ``use_prob`` weights, quantitative
traits (``hlaAssocQuant`` has permutations), and ``perm_p_adj`` as the stop rule of ``hlaAssocStepwise``."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .assoc import MODELS, _check_model, _check_perm, _Plan, _ptr
from .assocglm import COV0, FLAG_MAXIT, FLAG_RANK, MAX_COVAR, SLOTS, _base_model, _check_fit_control, _condition_list, _condition_tests, _design
from .assocomni import OMNIBUS_MODELS, _DeviceOmni, _design_sets, _partition_rows
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass

MAX_ROWS = 30                      # HIBAG_HIP_SCORE_MAX_ROWS

_exp = np.frompyfunc(math.exp, 1, 1)
_erfc = np.frompyfunc(math.erfc, 1, 1)


def chisq_sf_array(x, df: int) -> np.ndarray:
    """``assoc.chisq_sf`` of every element of ``x`` with one integer ``df``: the same operations in the same order (``exp`` and
    ``erfc`` are ``math``'s), so every element equals the scalar function's value; NaN for NaN or ``df < 1``."""
    x = np.asarray(x, np.float64)
    out = np.full(x.shape, np.nan)
    ok = ~np.isnan(x)
    if df < 1 or not ok.any():
        return out
    h = np.maximum(x[ok], 0.0) / 2.0
    if df % 2 == 0:
        term, total = np.ones_like(h), np.ones_like(h)
        for k in range(1, df // 2):
            term = term * h / k
            total = total + term
        out[ok] = _exp(-h).astype(np.float64) * total
        return out
    root = np.sqrt(h)
    tail = _erfc(root).astype(np.float64)
    if df > 1:
        term = root / (math.sqrt(math.pi) / 2.0)
        total = term
        for k in range(1, (df - 1) // 2):
            term = term * h / (k + 0.5)
            total = total + term
        tail = tail + _exp(-h).astype(np.float64) * total
    out[ok] = tail
    return out


class _DeviceScore(_DeviceOmni):
    """The tests of one cohort on the device, with a base model and its score tests on them (``hibag_hip_score``)."""

    _s = None
    n_score_rows = 0                    # rows of the last score_real_sets; 0: the handle's own rows are installed

    def score(self, covar: Optional[np.ndarray], weight: Optional[np.ndarray], maxit: int, epsilon: float) -> None:
        """The base model over the covariates [q, n_kept] and prior weights [n_kept]; ValueError for collinear covariates."""
        covar = None if covar is None or len(covar) == 0 else np.ascontiguousarray(covar, np.float64)
        weight = None if weight is None else np.ascontiguousarray(weight, np.float64)
        L = _lib.lib()
        self.score_close()
        self.n_basis = 1 + (0 if covar is None else covar.shape[0])
        self._s = L.hibag_hip_assoc_score_new(self._h, _ptr(covar), self.n_basis - 1, _ptr(weight), maxit, epsilon)
        if not self._s:
            msg = L.hibag_hip_last_error().decode("utf-8", "replace")
            if "collinear" in msg:
                raise ValueError("the covariates are collinear (the base model is rank-deficient)")
            raise _lib.HibagHipError(-1, msg)

    def score_close(self) -> None:
        if self._s:
            _lib.lib().hibag_hip_assoc_score_free(self._s)
            self._s = None

    def close(self) -> None:
        self.score_close()
        super().close()

    def score_base(self):
        """(coef, se [16] by the slots of ``hibag_hip_assoc_glm``, deviance, iterations, flags) of the base model."""
        coef, se, dev = np.empty(SLOTS), np.empty(SLOTS), np.empty(1)
        it, fl = np.empty(1, np.int32), np.empty(1, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_score_base(self._s, _ptr(coef), _ptr(se), _ptr(dev), _ptr(it), _ptr(fl)))
        return coef, se, float(dev[0]), int(it[0]), int(fl[0])

    def score_sets(self, sets: Sequence[Sequence[int]]):
        """Installs the sets of feature rows; (proj [rows, n_basis], S: per set [m, m], kept int32 [n_sets])."""
        start = np.zeros(len(sets) + 1, np.int32)
        start[1:] = np.cumsum([len(s) for s in sets])
        rows = np.ascontiguousarray([r for s in sets for r in s] or [0], np.int32)
        proj = np.empty((self.n_rows, self.n_basis))
        S = np.empty(max(sum(len(s) ** 2 for s in sets), 1))
        kept = np.empty(max(len(sets), 1), np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_score_sets(self._s, _ptr(start), _ptr(rows), len(sets), _ptr(proj), _ptr(S), _ptr(kept)))
        self.n_sets, self.n_score_rows = len(sets), 0
        out, at = [], 0
        for s in sets:
            out.append(S[at:at + len(s) ** 2].reshape(len(s), len(s)).copy())
            at += len(s) ** 2
        return proj, out, kept[:len(sets)]

    def score_real_sets(self, rows: np.ndarray, sets: Sequence[Sequence[int]]):
        """Installs sets over the real-valued rows [m, n_kept] in place of the handle's own; returns as ``score_sets``, proj
        [m, n_basis].  ``score_observed`` and ``score_resample`` then run over these rows."""
        rows = np.ascontiguousarray(rows, np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.n_kept:
            raise ValueError("rows must be a [m, n_kept] array")
        start = np.zeros(len(sets) + 1, np.int32)
        start[1:] = np.cumsum([len(s) for s in sets])
        idx = np.ascontiguousarray([r for s in sets for r in s] or [0], np.int32)
        proj = np.empty((len(rows), self.n_basis))
        S = np.empty(max(sum(len(s) ** 2 for s in sets), 1))
        kept = np.empty(max(len(sets), 1), np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_rscore_sets(self._s, _ptr(rows), len(rows), _ptr(start), _ptr(idx), len(sets), _ptr(proj),
                                                              _ptr(S), _ptr(kept)))
        self.n_sets, self.n_score_rows = len(sets), len(rows)
        out, at = [], 0
        for s in sets:
            out.append(S[at:at + len(s) ** 2].reshape(len(s), len(s)).copy())
            at += len(s) ** 2
        return proj, out, kept[:len(sets)]

    def score_observed(self):
        """(g [rows], stat [n_sets], df, flags int32 [n_sets]); the rows are those of the last install."""
        g, stat = np.empty(self.n_score_rows or self.n_rows), np.empty(self.n_sets)
        df, flags = np.empty(self.n_sets, np.int32), np.empty(self.n_sets, np.int32)
        _lib.check(_lib.lib().hibag_hip_assoc_score_observed(self._s, _ptr(g), _ptr(stat), _ptr(df), _ptr(flags)))
        return g, stat, df, flags

    def score_resample(self, seed: int, p0: int, n_perm: int) -> Tuple[np.ndarray, np.ndarray]:
        """(max_stat [n_perm, n_df], count_point int64 [n_sets]) of replicates p0 .. p0 + n_perm - 1."""
        n_df = _lib.lib().hibag_hip_assoc_score_n_df(self._s)
        if n_df < 0:
            _lib.check(n_df)
        max_stat = np.empty((n_perm, n_df), np.float64)
        count = np.empty(max(self.n_sets, 1), np.int64)
        _lib.check(_lib.lib().hibag_hip_assoc_score_resample(self._s, seed, p0, n_perm, _ptr(max_stat), _ptr(count)))
        return max_stat, count[:self.n_sets]

    def score_signs(self, seed: int, p0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n_kept), np.int8)
        _lib.check(_lib.lib().hibag_hip_assoc_score_signs(self._s, seed, p0, n, _ptr(out)))
        return out

    def score_ms(self) -> Tuple[float, float, float]:
        ms = np.zeros(3)
        _lib.check(_lib.lib().hibag_hip_assoc_score_ms(self._s, _ptr(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2])


class HlaAssocScoreResult:
    """The table of ``hlaAssocScore``: one entry per test in the order of ``hlaAssocTest`` or, with ``omnibus``, per partition
    of ``groups``.  ``name``; ``df``, the columns of the test that are not aliased; ``score_stat`` and ``score_p``, its
    chi-square tail with ``df`` degrees of freedom; ``flags`` (bit 0: the base model did not converge within ``maxit``, every
    value is NaN; bit 1: not tested -- a constant or aliased column, fewer than two carried levels --, NaN; bit 3: a column
    was dropped as aliased).  With ``omnibus`` also ``n_levels`` and ``reference`` as ``hlaAssocOmnibus`` reports them, else
    ``None``.  ``base`` is the base model as ``hlaAssocGlm`` reports it.  With replicates: ``perm_p`` (pointwise),
    ``perm_p_adj`` (family-wise, single-step min-P), ``max_stat`` [n_perm, k], every replicate's largest statistic among the
    tests of each of the k distinct ``df`` values ``max_stat_df``, ``min_p`` [n_perm], every replicate's smallest p-value,
    ``n_perm`` and ``seed``.  ``n_samp`` samples entered, ``n_case`` of them cases; ``n_excluded`` fell to the threshold."""

    def __init__(self, model: str, locus: str, omnibus: bool, name: List[str], df, score_stat, score_p, flags, base: Dict[str, object],
                 n_samp: int, n_case: int, n_excluded: int, n_levels=None, reference=None, n_perm: int = 0, seed: Optional[int] = None,
                 perm_p=None, perm_p_adj=None, max_stat=None, max_stat_df=None, min_p=None):
        self.model, self.locus, self.omnibus, self.name = model, locus, omnibus, name
        self.df, self.score_stat, self.score_p, self.flags, self.base = df, score_stat, score_p, flags, base
        self.n_samp, self.n_case, self.n_excluded = n_samp, n_case, n_excluded
        self.n_levels, self.reference = n_levels, reference
        self.n_perm, self.seed = n_perm, seed
        self.perm_p, self.perm_p_adj = perm_p, perm_p_adj
        self.max_stat, self.max_stat_df, self.min_p = max_stat, max_stat_df, min_p

    def to_table(self) -> Dict[str, np.ndarray]:
        """The columns ``df``, ``score.st``, ``score.p``, then ``perm.p`` and ``perm.p.adj`` when there were replicates; the
        rows are ``name``."""
        out: Dict[str, np.ndarray] = {"df": self.df, "score.st": self.score_stat, "score.p": self.score_p}
        if self.n_perm > 0:
            out["perm.p"], out["perm.p.adj"] = self.perm_p, self.perm_p_adj
        return out

    def __repr__(self):
        what = "partitions" if self.omnibus else "tests"
        return (f"HlaAssocScoreResult({self.model!r}, {len(self.name)} {what}, {len(self.base['name']) - 1} covariate columns, "
                f"{self.n_samp} samples with {self.n_case} cases, {self.n_perm} replicates)")


def _single_sets(model: str, rsum: np.ndarray, n: int) -> List[List[int]]:
    """Per device test the feature rows of its set, decided from the integer row sums as DESIGN.md section 23 item 6 decides
    them: a constant column is not tested (an empty set); ``genotype``: a dummy nobody carries is left out, and a test with no
    carrier or nobody without the allele is not tested."""
    if model == "genotype":
        out = []
        for het, hom in zip(rsum[0::2].tolist(), rsum[1::2].tolist()):
            t = len(out)
            out.append([] if (het == 0 and hom == 0) or het + hom == n else [2 * t + j for j, r in enumerate((het, hom)) if r > 0])
        return out
    top = (2 if model == "additive" else 1) * n
    return [[] if r in (0, top) else [t] for t, r in enumerate(rsum.tolist())]


def _min_p(max_stat: np.ndarray, dfs: Sequence[int]) -> np.ndarray:
    """Every replicate's smallest p-value from its largest statistics per df (a tail is monotone in the statistic, so this is
    the minimum over the tests); NaN where a replicate has no statistic."""
    if max_stat.shape[1] == 0:
        return np.full(len(max_stat), np.nan)
    p = np.stack([chisq_sf_array(max_stat[:, k], int(d)) for k, d in enumerate(dfs)], axis=1)
    out = np.where(np.isnan(p), np.inf, p).min(axis=1)
    return np.where(np.isinf(out), np.nan, out)


def hlaAssocScore(hla: HlaAlleleClass, y: Sequence, covariates=None, model: str = "dominant", prob_threshold: float = float("nan"),
                  use_prob: bool = False, groups: Optional[HlaAlleleGroups] = None, omnibus: bool = False,
                  condition: Optional[Sequence[str]] = None, n_perm: int = 0, seed: Optional[int] = None, maxit: int = 25,
                  epsilon: float = 1e-8, _backend=None) -> HlaAssocScoreResult:
    """Score tests of ``y ~ h + covariates`` against ``y ~ covariates``, logistic, for every test of ``hlaAssocGlm`` -- or, with
    ``omnibus``, every partition of ``hlaAssocOmnibus`` -- with family-wise p-values by multiplier resampling, on the device.

    * ``hla``, ``y``, ``covariates``, ``model``, ``prob_threshold``, ``use_prob``, ``groups``, ``maxit``, ``epsilon``: as
      ``hlaAssocGlm``; the base model ``y ~ covariates`` is the only fit.
    * ``omnibus=False``: ``hlaAssocGlm``'s list of tests, one column each (the two dummies for ``genotype``).
      ``omnibus=True`` needs ``groups``: one test per partition on ``hlaAssocOmnibus``'s design -- the carried levels without the
      most frequent one, at most 30 columns; ``genotype`` is a ValueError.
    * ``condition``: names of tests (without ``omnibus``), or of partitions and tests (with it), whose columns join the
      covariates, as in the corresponding entry; at most 12 covariate columns together.
    * ``n_perm > 0``: that many sign replicates of the residuals under ``seed`` (drawn and reported when ``None``):
      ``perm_p[t] = (1 + #{p: T[t][p] >= T[t]}) / (n_perm + 1)`` and the family-wise
      ``perm_p_adj[t] = (1 + #{p: min_p[p] <= score_p[t]}) / (n_perm + 1)`` with ``min_p[p]`` the replicate's smallest p-value
      over all tests.  With ``use_prob`` this is a ValueError: under prior weights the replicates' variance is not the model's
      ("Not built").

    A column that is constant, or a linear combination of the covariates and the columns before it, is dropped (flag bit 3, one
    degree of freedom less); a test left without columns has bit 1 and NaN.  A base model that did not converge gives every
    test bit 0 and NaN; a rank-deficient one is a ValueError.  (``_backend``: the tests' seam -- a class with the interface of
    ``_DeviceScore`` that stands in for the device.)"""
    omnibus = bool(omnibus)
    if omnibus:
        if model == "genotype":
            raise ValueError("the genotype coding is not built for the omnibus test: additive, dominant or recessive")
        _check_model(model, OMNIBUS_MODELS)
        if groups is None:
            raise ValueError("omnibus=True needs 'groups': one test per partition")
    else:
        _check_model(model)
    if groups is not None and not isinstance(groups, HlaAlleleGroups):
        raise TypeError("'groups' must be an HlaAlleleGroups")
    _check_fit_control(maxit, epsilon)
    n_perm, seed = _check_perm(n_perm, seed)
    if use_prob and n_perm > 0:
        raise ValueError("resampling is not built with use_prob (DESIGN.md section 28, 'Not built'): under prior weights the "
                         "replicates' variance is not the model's; threshold the calls with prob_threshold, or use n_perm=0")
    plan = _Plan(hla, y, prob_threshold, groups)
    cov_names, cov, weight = _design(plan, hla, covariates, use_prob)
    n_user = len(cov_names)
    per = 2 if model == "genotype" else 1
    condition = _condition_list(condition, "partition or test" if omnibus else "test")
    if omnibus:
        part_names, part_rows = list(groups.names), _partition_rows(plan, groups)
        for c in condition:
            if c not in part_names and c not in plan.names:
                raise ValueError(f"condition: {c!r} is neither a partition nor a test of this analysis")
        cond_rows: List[int] = []
    else:
        rows, cond_names = _condition_tests(plan, condition, per)
        cond_rows = [per * r + j for r in rows for j in range(per)]
        cov_names += cond_names

    backend = _DeviceScore if _backend is None else _backend
    with backend(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        rsum = dev.row_sums()
        n_levels = reference = None
        if omnibus:
            sets, ref, carried_n = _design_sets(part_rows, rsum)
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
            row_sets = [[part_rows[p][lv] for lv in s] for p, s in enumerate(sets)]
            wide = [part_names[p] for p, s in enumerate(row_sets) if len(s) > MAX_ROWS]
            if wide:
                raise ValueError(f"partition {wide[0]!r} has more than {MAX_ROWS} columns")
            n_levels = np.array(carried_n, np.int32)
            reference = [None if r < 0 else groups.levels[p][r] for p, r in enumerate(ref)]
        else:
            row_sets = _single_sets(model, np.asarray(rsum), plan.n_samp)
        q = len(cov_names)
        if q > MAX_COVAR:
            raise ValueError(f"{q} covariate columns ({q - n_user} conditioned columns included); at most {MAX_COVAR}")
        for row in cond_rows:
            cov = np.concatenate([cov, dev.feature_rows(row, 1).astype(np.float64)])
        dev.score(cov, weight, int(maxit), float(epsilon))
        b_coef, b_se, b_dev, b_it, b_fl = dev.score_base()
        dev.score_sets(row_sets)
        _, d_stat, d_df, d_flags = dev.score_observed()
        if n_perm > 0:
            max_stat, d_count = dev.score_resample(seed, 1, n_perm)

    if b_fl & FLAG_RANK:
        raise ValueError("the covariates are collinear (the base model is rank-deficient)")
    if omnibus:
        names, pick = part_names, (lambda a, fill=np.nan: np.asarray(a))
    else:
        names, pick = plan.names, plan.spread
    stat = pick(d_stat).astype(np.float64)
    df = pick(d_df, 0).astype(np.int32)
    flags = pick(d_flags, FLAG_RANK | (b_fl & FLAG_MAXIT)).astype(np.int32)
    score_p = np.full(len(stat), np.nan)
    for d in sorted(set(df[df > 0].tolist())):
        score_p[df == d] = chisq_sf_array(stat[df == d], d)
    base = _base_model(b_coef, b_se, b_dev, b_it, b_fl, [0] + list(range(COV0, COV0 + q)), cov_names)
    res = HlaAssocScoreResult(model, hla.locus, omnibus, list(names), df, stat, score_p, flags, base, plan.n_samp, plan.n_case,
                              plan.n_excluded, n_levels, reference)
    if n_perm > 0:
        dfs = sorted(set(np.asarray(d_df)[np.asarray(d_df) > 0].tolist()))
        assert max_stat.shape == (n_perm, len(dfs))
        min_p = _min_p(max_stat, dfs)
        nan = np.isnan(stat)
        order = np.sort(min_p[~np.isnan(min_p)])
        count_min = np.searchsorted(order, score_p, side="right")          # #{p: min_p[p] <= score_p[t]} (NaN: masked below)
        res.perm_p = np.where(nan, np.nan, (1 + pick(d_count, 0)) / (n_perm + 1))
        res.perm_p_adj = np.where(nan, np.nan, (1 + count_min) / (n_perm + 1))
        res.max_stat, res.max_stat_df, res.min_p = max_stat, np.array(dfs, np.int32), min_p
        res.n_perm, res.seed = n_perm, seed
    return res


__all__ = ["HlaAssocScoreResult", "hlaAssocScore"]
