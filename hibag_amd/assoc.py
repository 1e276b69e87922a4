"""``hlaAssocTest``: allele association tests of a case / control trait (``R/Association.R``), with permutation p-values.

One test per allele of the typed cohort -- and, with ``groups``, one per level of every partition of the alleles: the
two-digit and amino-acid analyses of ``hlaAssocTest.hlaAASeqClass`` --, each R's ``chisq.test`` and ``fisher.test`` of a
2 x 2 table (3 x 2 for the ``genotype`` model).  A locus is hundreds of correlated tests, so the p-value to report is the
family-wise one from permutations of the phenotype (single-step max-T, Westfall and Young): ``n_perm`` permutations give
``perm_p`` (pointwise) and ``perm_p_adj`` (family-wise).  Every permuted statistic is a function of one integer, the number
of case carriers, a dot product over samples; all tests under all permutations are one int8 Gram matrix on the device
(``hibag_hip_assoc_*``) with exact integer sums.  The result is defined exactly and does not depend
on panel sizes or on how the permutations are split over calls.

Not built: ``fisher_p`` of the ``genotype`` model (R's 3 x 2 network algorithm), which stays NaN.  The ``glm`` regression
with covariates and ``use.prob`` is ``hlaAssocGlm`` (assocglm.py); quantitative traits (R's t-test and ANOVA columns) are
``hlaAssocQuant`` (assocquant.py)."""

from __future__ import annotations

import ctypes as C
import math
import secrets
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .groups import HlaAlleleGroups
from .hibag import HlaAlleleClass
from .model import NA_INTEGER
from .train import hlaUniqueAllele

MODELS = ("dominant", "additive", "recessive", "genotype")
COUNT_NAMES = {"dominant": ("[-/-]", "[-/h,h/h]"), "additive": ("[-]", "[h]"), "recessive": ("[-/-,-/h]", "[h/h]"),
               "genotype": ("[-/-]", "[-/h]", "[h/h]")}
MAX_SAMPLES = 1 << 24


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_na(v) -> bool:
    return v is None or (isinstance(v, (float, np.floating)) and math.isnan(v))


def _labels(y, n: int) -> np.ndarray:
    """y as int32 0 / 1 [n]: 0 / 1 or bool as they are, else two distinct values, the smaller one the control."""
    y = list(np.asarray(y, dtype=object).ravel()) if not isinstance(y, (list, tuple)) else list(y)
    if len(y) != n:
        raise ValueError(f"'hla' and 'y' must have the same length ({n} samples, {len(y)} values of y)")
    if any(_is_na(v) for v in y):
        raise ValueError("y has missing values: subset the samples first (hlaAlleleSubset)")
    try:
        values = sorted(set(y))
    except TypeError:
        raise ValueError("the values of y cannot be ordered") from None
    if all(v in (0, 1) for v in values):       # (True == 1, False == 0)
        return np.array([int(v) for v in y], np.int32)
    if len(values) != 2:
        raise ValueError(f"y must be 0 / 1 or hold two distinct values, got {len(values)}")
    return np.array([int(v == values[1]) for v in y], np.int32)


def _check_model(model: str, models: Sequence[str] = MODELS) -> None:
    if model not in models:
        raise ValueError("'arg' should be one of " + ", ".join(f'"{m}"' for m in models))


def _check_perm(n_perm, seed) -> Tuple[int, Optional[int]]:
    """(n_perm, seed) as ints; the seed is drawn when there are permutations and none is given."""
    if isinstance(n_perm, bool) or not isinstance(n_perm, (int, np.integer)) or n_perm < 0:
        raise ValueError("n_perm must be an integer >= 0")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64):
        raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
    if n_perm > 0 and seed is None:
        seed = secrets.randbits(64)
    return int(n_perm), None if seed is None else int(seed)


class _Plan:
    """What the device is told and how its tests are called: ``sel``, the indices of the samples left after the call
    threshold that have two known alleles, their allele indices into ``alleles``, their labels (``y=None``, an entry without
    a case / control label: all 0), the partitions restricted to ``alleles``, and per test of the RESULT its name and its row
    among the device's tests (-1: a level that no allele of the data belongs to, which the device does not know and whose
    statistics are NaN; ``spread`` maps the device's arrays onto the result's tests)."""

    def __init__(self, hla: HlaAlleleClass, y, prob_threshold: float, groups: Optional[HlaAlleleGroups]):
        if not isinstance(hla, HlaAlleleClass):
            raise TypeError('inherits(hla, "hlaAlleleClass") is not TRUE')
        n_all = len(hla.sample_id)
        lab = np.zeros(n_all, np.int32) if y is None else _labels(y, n_all)
        h1, h2 = list(hla.allele1), list(hla.allele2)
        keep = np.ones(n_all, bool)
        if isinstance(prob_threshold, bool) or not isinstance(prob_threshold, (int, float, np.integer, np.floating)):
            raise TypeError("is.numeric(prob.threshold) is not TRUE")
        if math.isfinite(prob_threshold):
            if hla.prob is None:
                raise ValueError("No posterior probability in 'hla' ('hla.prob' should be available).")
            with np.errstate(invalid="ignore"):
                keep = np.asarray(hla.prob, np.float64) >= float(prob_threshold)      # (NaN: excluded)
        self.n_excluded = int(n_all - keep.sum())
        known = np.array([not _is_na(a) and not _is_na(b) for a, b in zip(h1, h2)], bool) if n_all else np.zeros(0, bool)
        sel = np.flatnonzero(keep & known)
        if sel.size == 0:
            raise ValueError("no sample with two known alleles is left")
        if sel.size > MAX_SAMPLES:
            raise ValueError(f"{sel.size} samples; at most 2^24")
        self.sel = sel
        self.n_samp = int(sel.size)
        self.alleles = hlaUniqueAllele([h1[i] for i in sel] + [h2[i] for i in sel])
        pos = {a: i for i, a in enumerate(self.alleles)}
        self.a1 = np.array([pos[h1[i]] for i in sel], np.int32)
        self.a2 = np.array([pos[h2[i]] for i in sel], np.int32)
        self.y = np.ascontiguousarray(lab[sel])
        self.n_case = int(self.y.sum())
        self.names = list(self.alleles)
        self.row = list(range(len(self.alleles)))
        self.group_of = None
        if groups is not None:
            if not isinstance(groups, HlaAlleleGroups):
                raise TypeError("'groups' must be an HlaAlleleGroups")
            at = {a: i for i, a in enumerate(groups.alleles)}
            unknown = [a for a in self.alleles if a not in at]
            if unknown:
                raise ValueError(f"allele {unknown[0]!r} of the data is not among the alleles of 'groups'")
            self.group_of = np.ascontiguousarray(groups.group_of[:, [at[a] for a in self.alleles]], np.int32)
            nxt = len(self.alleles)
            for q in range(groups.n_part):
                known_levels = int(self.group_of[q].max()) + 1          # the device numbers levels 0 .. the largest id in use
                for lv, name in enumerate(groups.levels[q]):
                    self.names.append(f"{groups.names[q]}:{name}")
                    self.row.append(nxt + lv if lv < known_levels else -1)
                nxt += known_levels
            self.n_device_tests = nxt
        else:
            self.n_device_tests = len(self.alleles)

    def spread(self, a, fill=np.nan) -> np.ndarray:
        """The per-device-test array ``a`` [n_device_tests, ...] per test of the result, ``fill`` for a level unknown to the
        device (no allele of the data belongs to it, so it has no carrier)."""
        a = np.asarray(a)
        row = np.array(self.row, np.int64)
        return np.where((row >= 0).reshape((-1,) + (1,) * (a.ndim - 1)), a[np.maximum(row, 0)], fill)


def _columns(model: str, table: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's count columns and ``%.`` columns from the integer tables [n_test, 6] (rows x (control, case)):
    the units per row, and ``round(100 * cases / units, 1)``, NaN for an empty row."""
    k = len(COUNT_NAMES[model])
    cells = np.asarray(table, np.int64).reshape(-1, 3, 2)[:, :k, :]
    counts = cells.sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = np.round(100.0 * (cells[:, :, 1] / counts), 1)
    pct[counts == 0] = np.nan
    return counts, pct


def chisq_sf(x: float, df: int) -> float:
    """The upper tail of chi-square with an integer ``df`` >= 1, in closed form: for even df
    ``exp(-x/2) sum_{k < df/2} (x/2)^k / k!``; for odd df ``erfc(sqrt(x/2))`` plus the half-integer terms
    ``exp(-x/2) sum_{k=1}^{(df-1)/2} (x/2)^(k-1/2) / Gamma(k+1/2)``.  Every term is positive: nothing cancels."""
    if math.isnan(x) or df < 1:
        return math.nan
    h = max(x, 0.0) / 2.0
    if df % 2 == 0:
        term, total = 1.0, 1.0
        for k in range(1, df // 2):
            term = term * h / k
            total = total + term
        return math.exp(-h) * total
    tail = math.erfc(math.sqrt(h))
    if df == 1:
        return tail
    term = math.sqrt(h) / (math.sqrt(math.pi) / 2.0)       # (x/2)^(1/2) / Gamma(3/2)
    total = term
    for k in range(1, (df - 1) // 2):
        term = term * h / (k + 0.5)
        total = total + term
    return tail + math.exp(-h) * total


def _chisq_p(stat: np.ndarray, df: int) -> np.ndarray:
    """``chisq_sf`` of every statistic: for 1 and 2 degrees of freedom erfc(sqrt(st / 2)) and exp(-st / 2)."""
    return np.array([chisq_sf(float(st), df) for st in stat], np.float64)


def _fisher_p(table: np.ndarray) -> np.ndarray:
    """R's two-sided ``fisher.test`` of 2 x 2 tables [n_test, 6] (cells 0-3): with the margins fixed, the probabilities of
    all tables not more probable than the observed one (within the factor 1 + 1e-7), from ``lgamma``.  NaN for a table
    with an empty margin (R's ``fisher.test`` refuses a factor with one level)."""
    table = np.asarray(table, np.int64)
    out = np.full(len(table), np.nan)
    if not len(table):
        return out
    top = int(table[:, :4].sum(axis=1).max())
    lg = np.array([math.lgamma(v + 1.0) for v in range(top + 1)], np.float64)       # lg[v] = log v!
    for t, (x00, x01, x10, x11) in enumerate(table[:, :4].tolist()):
        r1, r2, c1 = x10 + x11, x00 + x01, x01 + x11
        N = r1 + r2
        c2 = N - c1
        if r1 == 0 or r2 == 0 or c1 == 0 or c2 == 0:
            continue
        lo, hi = max(0, c1 - r2), min(r1, c1)
        k = np.arange(lo, hi + 1)
        logd = ((lg[r1] - lg[k] - lg[r1 - k]) + (lg[r2] - lg[c1 - k] - lg[r2 - c1 + k])) - (lg[N] - lg[c1] - lg[c2])
        d = np.exp(logd - logd.max())
        sel = d <= d[x11 - lo] * (1.0 + 1e-7)
        out[t] = np.cumsum(d[sel])[-1] / np.cumsum(d)[-1]       # (cumsum: added one by one, in the order of the support)
    return out


class _DeviceAssoc:
    """The tests of one cohort on the device (``hibag_hip_assoc``)."""

    def __init__(self, a1: np.ndarray, a2: np.ndarray, y: np.ndarray, n_allele: int, group_of: Optional[np.ndarray], model: int):
        self._keep = [np.ascontiguousarray(a1, np.int32), np.ascontiguousarray(a2, np.int32), np.ascontiguousarray(y, np.int32),
                      None if group_of is None else np.ascontiguousarray(group_of, np.int32)]
        a1, a2, y, g = self._keep
        L = _lib.lib()
        self._h = L.hibag_hip_assoc_new(_ptr(a1), _ptr(a2), _ptr(y), len(a1), n_allele, _ptr(g), 0 if g is None else g.shape[0], model)
        if not self._h:
            raise _lib.HibagHipError(-1, L.hibag_hip_last_error().decode("utf-8", "replace"))
        self.n_tests = L.hibag_hip_assoc_n_tests(self._h)
        self.n_rows = self.n_tests * (2 if MODELS[model] == "genotype" else 1)       # the feature rows
        self.n_kept = int(np.count_nonzero((a1 != NA_INTEGER) & (a2 != NA_INTEGER)))

    def close(self) -> None:
        if self._h:
            _lib.lib().hibag_hip_assoc_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def observed(self) -> Tuple[np.ndarray, np.ndarray]:
        stat = np.empty(self.n_tests, np.float64)
        table = np.empty((self.n_tests, 6), np.int64)
        _lib.check(_lib.lib().hibag_hip_assoc_observed(self._h, _ptr(stat), _ptr(table)))
        return stat, table

    def permute(self, seed: int, perm0: int, n_perm: int) -> Tuple[np.ndarray, np.ndarray]:
        max_stat = np.empty(n_perm, np.float64)
        count = np.empty(self.n_tests, np.int64)
        _lib.check(_lib.lib().hibag_hip_assoc_permute(self._h, seed, perm0, n_perm, _ptr(max_stat), _ptr(count)))
        return max_stat, count

    def labels(self, seed: int, perm0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n_kept), np.int8)
        _lib.check(_lib.lib().hibag_hip_assoc_labels(self._h, seed, perm0, n, _ptr(out)))
        return out


class HlaAssocResult:
    """The table of ``hlaAssocTest``, one entry per test in test order (the alleles, then the partitions of ``groups`` in
    order, their levels in order): ``name``; ``counts`` int64 [n_test, k] and ``pct`` [n_test, k] under ``count_names``
    (the reference's ``[-/-]``, ``[-/h,h/h]``, ... columns: the units per genotype class, and the percentage of cases among
    them, NaN where the class is empty); ``chisq_st``, ``chisq_p``, ``fisher_p``; with permutations ``perm_p`` (pointwise),
    ``perm_p_adj`` (family-wise, single-step max-T), ``max_stat`` [n_perm], ``n_perm`` and ``seed``.  ``n_samp`` samples
    entered the tests, ``n_case`` of them cases; ``n_excluded`` fell to the call threshold."""

    def __init__(self, model: str, locus: str, name: List[str], counts, pct, chisq_st, chisq_p, fisher_p, n_samp: int, n_case: int,
                 n_excluded: int, n_perm: int = 0, seed: Optional[int] = None, perm_p=None, perm_p_adj=None, max_stat=None):
        self.model, self.locus, self.name = model, locus, name
        self.count_names = COUNT_NAMES[model]
        self.counts, self.pct = counts, pct
        self.chisq_st, self.chisq_p, self.fisher_p = chisq_st, chisq_p, fisher_p
        self.n_samp, self.n_case, self.n_excluded = n_samp, n_case, n_excluded
        self.n_perm, self.seed = n_perm, seed
        self.perm_p, self.perm_p_adj, self.max_stat = perm_p, perm_p_adj, max_stat

    def to_table(self) -> Dict[str, np.ndarray]:
        """The columns under the reference's names, in its order (``[-/-]``, ..., ``%.[-/-]``, ..., ``chisq.st``,
        ``chisq.p``, ``fisher.p``), then ``perm.p`` and ``perm.p.adj`` when there were permutations; the rows are ``name``."""
        out: Dict[str, np.ndarray] = {}
        for j, c in enumerate(self.count_names):
            out[c] = self.counts[:, j]
        for j, c in enumerate(self.count_names):
            out["%." + c] = self.pct[:, j]
        out["chisq.st"], out["chisq.p"], out["fisher.p"] = self.chisq_st, self.chisq_p, self.fisher_p
        if self.n_perm > 0:
            out["perm.p"], out["perm.p.adj"] = self.perm_p, self.perm_p_adj
        return out

    def __repr__(self):
        return (f"HlaAssocResult({self.model!r}, {len(self.name)} tests, {self.n_samp} samples with {self.n_case} cases, "
                f"{self.n_perm} permutations)")


def _perm_p(stat_obs: np.ndarray, count_point: np.ndarray, max_stat: np.ndarray, n_perm: int) -> Tuple[np.ndarray, np.ndarray]:
    """(1 + #{p: stat[t][p] >= stat_obs[t]}) / (n_perm + 1) and the same with max_stat[p] in place of stat[t][p]; NaN where
    the observed statistic is NaN."""
    order = np.sort(max_stat[~np.isnan(max_stat)])
    count_max = len(order) - np.searchsorted(order, stat_obs, side="left")          # (NaN sorts last: count 0, masked below)
    nan = np.isnan(stat_obs)
    perm_p = np.where(nan, np.nan, (1 + count_point) / (n_perm + 1))
    perm_p_adj = np.where(nan, np.nan, (1 + count_max) / (n_perm + 1))
    return perm_p, perm_p_adj


def _attach_perm(res, plan: _Plan, stat: np.ndarray, max_stat: np.ndarray, d_count: np.ndarray, n_perm: int, seed: int) -> None:
    """The permutation columns of a result from the device's ``max_stat`` and per-device-test counts."""
    res.perm_p, res.perm_p_adj = _perm_p(stat, plan.spread(d_count, 0), max_stat, n_perm)
    res.max_stat, res.n_perm, res.seed = max_stat, n_perm, seed


def hlaAssocTest(hla: HlaAlleleClass, y: Sequence, model: str = "dominant", prob_threshold: float = float("nan"),
                 groups: Optional[HlaAlleleGroups] = None, n_perm: int = 0, seed: Optional[int] = None) -> HlaAssocResult:
    """Association tests of the alleles of ``hla`` with the case / control label ``y`` (``hlaAssocTest`` of the reference
    for a two-level trait without covariates), on the device.

    * ``hla``: a result of a predict entry, or ``hlaAllele(...)``.  ``y``: one value per sample, 0 / 1 or bool, or any two
      distinct values (the smaller one is the control); a missing value is a ValueError.
    * A finite ``prob_threshold`` drops the samples with ``prob < prob_threshold`` (``n_excluded`` of them); samples with
      an unknown allele are dropped as well.
    * ``model``: ``dominant`` (carrier or not), ``additive`` (chromosomes: 2 n units, each with its person's label),
      ``recessive`` (homozygous or not) -- 2 x 2 tables, Yates-corrected chi-square as R's ``chisq.test`` -- or ``genotype``
      (none / het / hom, 3 x 2, no correction).
    * One test per allele of ``hlaUniqueAllele`` over the kept samples; with ``groups`` also one per level of every
      partition (named ``partition:level``), "an allele of the sample is in the level" in place of "is the allele".
      ``groups.alleles`` is matched by name; an allele of the data it does not hold is a ValueError.  A level that no
      kept sample carries stays in the table with NaN statistics.
    * ``n_perm > 0``: permutation p-values from ``n_perm`` permutations of the labels under ``seed`` (drawn and reported
      when ``None``): ``perm_p[t] = (1 + #{p: stat[t][p] >= stat[t]}) / (n_perm + 1)`` and the family-wise
      ``perm_p_adj[t]`` with the permutation's largest statistic over all tests in place of ``stat[t][p]``.

    Not built: ``fisher_p`` for the ``genotype`` model, which is NaN; the ``glm`` regression with covariates and ``use.prob``
    is ``hlaAssocGlm``, a quantitative trait ``hlaAssocQuant``.  The statistics, the generator and the counts are defined in DESIGN.md
    section 20."""
    _check_model(model)
    n_perm, seed = _check_perm(n_perm, seed)
    plan = _Plan(hla, y, prob_threshold, groups)
    with _DeviceAssoc(plan.a1, plan.a2, plan.y, len(plan.alleles), plan.group_of, MODELS.index(model)) as dev:
        assert dev.n_tests == plan.n_device_tests
        d_stat, d_table = dev.observed()
        if n_perm > 0:
            max_stat, d_count = dev.permute(seed, 1, n_perm)
    stat = plan.spread(d_stat)
    unit = 2 if model == "additive" else 1
    table = plan.spread(d_table, [unit * (plan.n_samp - plan.n_case), unit * plan.n_case, 0, 0, 0, 0])
    counts, pct = _columns(model, table)
    fisher = _fisher_p(table) if model != "genotype" else np.full(len(stat), np.nan)
    res = HlaAssocResult(model, hla.locus, plan.names, counts, pct, stat, _chisq_p(stat, 2 if model == "genotype" else 1), fisher,
                         plan.n_samp, plan.n_case, plan.n_excluded)
    if n_perm > 0:
        _attach_perm(res, plan, stat, max_stat, d_count, n_perm, seed)
    return res


__all__ = ["HlaAssocResult", "hlaAssocTest"]
