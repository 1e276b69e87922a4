"""CPU restatement of hlaAssocInteract for the tests: DESIGN.md section 27 in numpy, written from the definitions.

A *term* is a feature row or the product of two (``term_column``: formed in integers); ``glm_terms`` is what
``hibag_hip_assoc_glm_terms`` returns -- the fit of section 23 items 3-5 with the drop rule of section 26 item 2
(``assocomni_reference.fit``: factorisation order intercept, covariates, terms in slot order) for every fit record and the base
model, by slot, with the rules of section 27 item 3 for terms that nobody carries --, ``row_gram`` what
``hibag_hip_assoc_row_gram`` returns, ``Backend`` both behind the interface ``hibag_amd.associnteract`` drives.  Dtype-generic
like its siblings; the samples, tests, feature rows and cohorts are those of tests/assocomni_reference.py."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
import assocomni_reference as O

MODELS = ("additive", "dominant", "recessive")
SLOTS, TERMS, COV0, MAX_COVAR = 16, 3, 4, 11
MAXIT_BIT, RANK_BIT, BOUNDARY_BIT, ALIASED_BIT = 1, 2, 4, 8
UNUSED = (-1, -1)


def term_column(F, a, b):
    """int64 [n]: row a, or the product of rows a and b."""
    return F[a].astype(np.int64) if b < 0 else F[a].astype(np.int64) * F[b].astype(np.int64)


def row_gram(F, row0, n_rows):
    R = F[row0:row0 + n_rows].astype(np.int64)
    return R @ R.T


def glm_terms(F, terms, covar, weight, y, maxit=25, epsilon=1e-8, dtype=np.float64):
    """What hibag_hip_assoc_glm_terms returns from the feature rows F [rows, n] and the fit records terms [n_fits, 3, 2]: dict
    of coef, se [n_fits + 1, 16] by slot (float64), deviance, iterations, flags, df_h [n_fits + 1], and crit / ratios, lists
    per fit; the last fit is the base model."""
    n = F.shape[1]
    covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
    q = len(covar)
    assert q <= MAX_COVAR
    wt = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    terms = np.asarray(terms, np.int64).reshape(-1, TERMS, 2)
    n_fit = len(terms) + 1
    out = dict(coef=np.full((n_fit, SLOTS), np.nan), se=np.full((n_fit, SLOTS), np.nan), deviance=np.full(n_fit, np.nan),
               iterations=np.zeros(n_fit, np.int32), flags=np.zeros(n_fit, np.int32), df_h=np.zeros(n_fit, np.int32),
               crit=[[] for _ in range(n_fit)], ratios=[[] for _ in range(n_fit)])
    for f, rec in enumerate([[tuple(t) for t in r] for r in terms.tolist()] + [[UNUSED] * TERMS]):
        used = [(j, a, b) for j, (a, b) in enumerate(rec) if a >= 0]
        assert all(-1 <= a < len(F) and -1 <= b < len(F) and (a >= 0 or b < 0) for a, b in rec)
        assert len({(a, -1) if b < 0 else (min(a, b), max(a, b)) for _, a, b in used}) == len(used)
        cols = [(j, term_column(F, a, b)) for j, a, b in used]
        carried = [(j, c) for j, c in cols if c.sum() > 0]                    # a term nobody carries is left out before the fit
        if f < len(terms) and not carried:
            out["flags"][f] = RANK_BIT
            continue
        slots = [0] + [1 + j for j, _ in carried] + list(range(COV0, COV0 + q))
        X = np.stack([np.ones(n)] + [c.astype(np.float64) for _, c in carried] + list(covar), axis=1)
        res = O.fit(X, len(carried), y, wt, maxit, epsilon, dtype)
        out["coef"][f, slots] = np.asarray(res["coef"], np.float64)
        out["se"][f, slots] = np.asarray(res["se"], np.float64)
        out["deviance"][f] = float(res["deviance"])
        out["iterations"][f], out["df_h"][f] = res["iterations"], res["df_h"]
        out["flags"][f] = res["flags"] | (ALIASED_BIT if len(carried) < len(cols) else 0)
        out["crit"][f], out["ratios"][f] = res["crit"], res["ratios"]
    return out


class Backend(O.Backend):
    """The restatement behind the interface of hibag_amd.associnteract._DeviceInteract
    (``hlaAssocInteract(..., _backend=Backend)``)."""

    LOG = []          # (crit, ratios) of every call, for the safety conditions of tests/test_associnteract_host.py

    def row_gram(self, row0, n_rows):
        return row_gram(self.A.F, row0, n_rows).astype(np.int32)

    def glm_terms(self, terms, covar, weight, maxit, epsilon):
        r = glm_terms(self.A.F, terms, covar, weight, self.A.y, maxit, epsilon, self.dtype)
        Backend.LOG.append((r["crit"], r["ratios"]))
        return r["coef"], r["se"], r["deviance"], r["iterations"], r["flags"], r["df_h"]


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
# The cohorts, kept samples and partitions of tests/assocomni_reference.py (40 / 255 / 256 / 257 / 1000 kept samples), with
# 0 / 1 / 5 / 11 / 6 covariates: 11 is the most that stands beside three term slots.
CASES, KEPT, analysis = O.CASES, O.KEPT, O.analysis
CASE_Q = {"n40": 0, "n255": 1, "n256": 5, "n257": 11, "n1000": 6}


def main(a, b):
    return [(a, -1), (b, -1), UNUSED]


def full(a, b):
    return [(a, -1), (b, -1), (a, b)]


def run_fits(case, model):
    """The fit records of a device run, [n_fits, 3, 2]: the main and the full fit of the pairs of the four most frequent
    alleles; fits of one plain term in slot 1, in slot 2 and in slot 3; three plain terms; a product alone; a product
    beside one of its factors only; the levels 0 of p2 and p3 with their product (carried under every model); allele 0
    with the level of p2 that holds it (``dominant`` and ``recessive``: the product IS allele 0's column, aliased exactly);
    the first pair of carried alleles that nobody carries together, main effects and product (``recessive``: every pair);
    a record with three unused terms; and, where the cohort has it, a row nobody carries beside a carried one."""
    A, _, _, part_rows = analysis(case, model)
    n_allele = CASES[case][1]
    F = A.F.astype(np.int64)
    fits = []
    for a in range(4):
        for b in range(a + 1, 4):
            fits += [main(a, b), full(a, b)]
    fits += [[(0, -1), UNUSED, UNUSED], [UNUSED, (1, -1), UNUSED], [UNUSED, UNUSED, (2, -1)], [(2, -1), (0, -1), (1, -1)]]
    fits += [[(0, 1), UNUSED, UNUSED], [(1, -1), UNUSED, (1, 0)]]
    p2_0, p3_0 = part_rows[0][0], part_rows[1][0]
    fits += [main(p2_0, p3_0), full(p3_0, p2_0)]
    fits += [full(0, p2_0)]
    apart = [(a, b) for a in range(n_allele) for b in range(a + 1, n_allele)
             if A.rsum[a] > 0 and A.rsum[b] > 0 and int(F[a] @ F[b]) == 0]
    if apart:
        fits += [full(*apart[0])]
    fits += [[UNUSED] * TERMS]
    if CASES[case][3]:
        gap = part_rows[4]
        assert A.rsum[gap[1]] == 0
        fits += [[(gap[1], -1), (0, -1), UNUSED], [(gap[1], -1), UNUSED, UNUSED]]
    return np.array(fits, np.int32)


# every (case, model, q, weighted, maxit) whose fits tests/test_hip_associnteract.py compares with the device;
# tests/test_associnteract_host.py asserts the safety conditions for each of them
DEVICE_RUNS = [(case, "additive", CASE_Q[case], False, 25) for case in CASES] + \
    [("n1000", "additive", 11, False, 25), ("n1000", "additive", 0, False, 25),
     ("n257", "dominant", 11, False, 25), ("n257", "recessive", 11, False, 25),
     ("n257", "additive", 11, False, 2), ("n257", "additive", 11, True, 25)]

_CACHE = {}


def reference(case, model, q, weighted=False, maxit=25, dtype=np.float64):
    """glm_terms of a device run, computed once per process and shared (callers do not modify it)."""
    key = (case, model, q, weighted, maxit, np.dtype(dtype).name)
    if key not in _CACHE:
        A, covar, prob, _ = analysis(case, model)
        _CACHE[key] = glm_terms(A.F, run_fits(case, model), covar[:q], prob if weighted else None, A.y, maxit, 1e-8, dtype)
    return _CACHE[key]


gaps = O.gaps           # est in units of max(|est|, se), se and deviance relative, over the fits without the rank bit


def tolerance_of(r, rl):
    """100 x the largest difference between the float64 and the longdouble restatement of the same fits, at least 1e-12."""
    assert np.array_equal(r["flags"], rl["flags"]) and np.array_equal(r["iterations"], rl["iterations"])
    assert np.array_equal(r["df_h"], rl["df_h"]) and np.array_equal(np.isnan(r["coef"]), np.isnan(rl["coef"]))
    return max(100.0 * max(gaps(r, rl)), 1e-12)


def tolerance(case, model, q, weighted=False, maxit=25):
    return tolerance_of(reference(case, model, q, weighted, maxit), reference(case, model, q, weighted, maxit, np.longdouble))


def hla_of(case):
    """The case's cohort as hlaAssocInteract takes it: (hla with ``prob``, y, groups, covar [n, 29])."""
    return O.hla_of(case)


# the end-to-end calls of tests/test_hip_associnteract.py, (case, covariates, keywords): the default pairs of the 257-sample
# cohort, and explicit pairs -- alleles and partition levels -- of the 1000-sample cohort, dominant, with prior weights,
# conditioned on an allele (pair 5: the product is the first allele's own column; pair 6: nobody carries gap.1)
END_TO_END = [("n257", 5, {}),
              ("n1000", 6, {"pairs": [("01:01", "02:01"), ("03:01", "p3:p3.1"), ("p2:p2.0", "p3:p3.0"), ("02:01", "05:01"),
                                      ("04:01", "p5:p5.2"), ("01:01", "p2:p2.0"), ("06:01", "gap:gap.1")],
                            "model": "dominant", "use_prob": True, "condition": ["03:01"], "min_both": 2})]


def planted(n=1500, n_allele=8, seed=31):
    """(hla, y, covar [n, 2], names): a cohort whose trait has main effects of alleles 0, 1 and 2 and an interaction of the
    alleles 1 and 2 (per copy of each: the dosage product)."""
    rng = np.random.default_rng(seed)
    w = 0.8 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    covar = rng.standard_normal((2, n))
    d = [(a == k).sum(axis=1) for k in range(3)]
    eta = -0.6 + 0.3 * d[0] - 0.4 * d[1] + 0.3 * d[2] + 2.0 * d[1] * d[2] + 0.2 * covar[0]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    hla, names, _ = AR.hla_of(a[:, 0], a[:, 1], rng.uniform(0.3, 1.0, n), n_allele)
    return hla, y, covar.T, names
