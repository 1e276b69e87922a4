"""The hard cohorts of tests/test_assoc_hard_host.py (CPU) and tests/test_hip_assoc_hard.py (GPU): separated and
monotone-likelihood fits for hibag_hip_assoc_glm and hibag_hip_assoc_cox, in plain numpy with fixed
seeds.  A cohort is a handful of ordinary alleles (0 .. 3, drawn from frequencies 0.4 / 0.3 / 0.2 / 0.1) plus one allele per
hard feature row, planted on chosen samples; ``GLM_ROWS`` / ``COX_ROWS`` name the hard alleles and say what each is.  A RUN is
a cohort with a model, covariates and controls; ``GLM_RUNS`` / ``COX_RUNS`` list every run whose fits the device tests
compare, ``glm_reference`` / ``cox_reference`` give a run's restatement (computed once per process, shared, read-only) and
``glm_tolerances`` / ``cox_tolerances`` the per-fit tolerances of the project's rule."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
import assocglm_reference as G
import assocsurv_reference as S

N_ORDINARY = 4
SIZES = (40, 255, 257)
LEFT_OUT_ABOVE = 1e-6                  # a fit whose own tolerance exceeds this has est and se left out of the value comparison


def _ordinary(rng, n):
    return rng.choice(N_ORDINARY, (n, 2), p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)


def _take(free, want, k):
    """The first k samples of ``free`` (a boolean mask, updated) that ``want`` allows."""
    idx = np.flatnonzero(free & want)[:k]
    assert len(idx) == k, "the cohort is too small for its hard rows"
    free[idx] = False
    return idx


# ---- logistic regression ----------------------------------------------------------------------------------------------------
# name -> what the allele's carriers are; the alleles come in this order after the ordinary ones
GLM_ROWS = {
    "all_cases": "six carriers (four at n = 40), all of them cases: complete separation, the estimate runs to +inf",
    "all_controls": "six carriers (four at n = 40), all of them controls: the estimate runs to -inf",
    "single_case": "one carrier, a case",
    "quasi": "five case carriers and one control: quasi-separation, a finite maximum",
    "zero_weight": "carriers that all have prior weight 0 in a weighted run: the host keeps the row, the kernel meets A_jj = 0",
    "tiny_weight": "two case and two control carriers, prior weight 1e-12 each in a weighted run",
    "het_sep": "(n > 40) six heterozygous carriers, all cases; four homozygous carriers, two cases and two controls",
    "hom_sep": "(n > 40) six heterozygous carriers, three cases and three controls; three homozygous carriers, all cases",
}
# beside them: the carriers of both ordinary alleles 2 and 3 are all cases (an interaction product carried by cases only),
# and level 1 of the cohort's one partition is {allele 1, all_cases}: its row differs from allele 1's on separated samples only

GLM_COVARS = {
    "q0": "no covariates",
    "q2": "two standard normal covariates",
    "sep": "two normal covariates and one that separates y by itself: the base model and every fit are separated",
    "big": "two normal covariates and one of scale 1e3",
}

_cache = {}


def glm_cohort(case):
    """dict a1, a2, y, n_allele, names (allele index -> hard row name), weight [n], covar (kind -> [q, n]) of ``case``:
    "n40", "n255", "n257", or "eq_y", 40 samples whose allele 4 is carried by the cases and by nobody else (the feature
    equals y)."""
    if ("glm", case) in _cache:
        return _cache[("glm", case)]
    n = 40 if case == "eq_y" else int(case[1:])
    rng = np.random.default_rng(1000 + n + (case == "eq_y"))
    a = _ordinary(rng, n)
    z = rng.standard_normal((2, n))
    eta = -0.2 + 0.8 * (a == 0).any(axis=1) - 0.7 * (a == 1).any(axis=1) + 0.4 * z[0]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    weight = rng.uniform(0.3, 1.0, n)
    names = {}
    if case != "eq_y":                                           # the carriers of both alleles 2 and 3 are cases, three at least
        a[:3] = (2, 3)
        y[((a == 2).any(axis=1)) & ((a == 3).any(axis=1))] = 1
    case_, ctrl = y == 1, y == 0
    if case == "eq_y":
        a[case_, 0] = N_ORDINARY
        names[N_ORDINARY] = "equals_y"
    else:
        free = ~(((a == 2).any(axis=1)) & ((a == 3).any(axis=1)))
        k = 4 if n == 40 else 6
        plant = [("all_cases", _take(free, case_, k), None), ("all_controls", _take(free, ctrl, k), None),
                 ("single_case", _take(free, case_, 1), None),
                 ("quasi", np.r_[_take(free, case_, 5), _take(free, ctrl, 1)], None)]
        zw = _take(free, case_ | ctrl, 3)
        tw = np.r_[_take(free, case_, 2), _take(free, ctrl, 2)]
        plant += [("zero_weight", zw, None), ("tiny_weight", tw, None)]
        weight[zw], weight[tw] = 0.0, 1e-12
        if n > 40:
            plant += [("het_sep", _take(free, case_, 6), np.r_[_take(free, case_, 2), _take(free, ctrl, 2)]),
                      ("hom_sep", np.r_[_take(free, case_, 3), _take(free, ctrl, 3)], _take(free, case_, 3))]
        for i, (name, het, hom) in enumerate(plant):
            k = N_ORDINARY + i
            names[k] = name
            a[het, 1] = k
            if hom is not None:
                a[hom, 0] = a[hom, 1] = k
    sep = (2.0 * y - 1.0) * (1.0 + np.abs(rng.standard_normal(n)))
    big = 1e3 * (rng.standard_normal(n) + 0.3 * y)
    covar = {"q0": np.zeros((0, n)), "q2": z, "sep": np.vstack([z, sep]), "big": np.vstack([z, big])}
    n_allele = N_ORDINARY + len(names)
    # one partition: level 1 holds the ordinary allele 1 and the first hard allele (all_cases, or equals_y), level 0 the rest
    g = np.zeros((1, n_allele), np.int32)
    g[0, [1, N_ORDINARY]] = 1
    c = dict(a1=np.ascontiguousarray(a[:, 0]), a2=np.ascontiguousarray(a[:, 1]), y=y, n_allele=n_allele, names=names, weight=weight,
             covar=covar, g=g, level_rows=(n_allele, n_allele + 1))
    _cache[("glm", case)] = c
    return c


# (cohort, model, covariates, weighted, maxit, epsilon).  The default controls (25, 1e-8) stop a separated fit near |eta| = 25,
# before the |eta| > 30 substitution; the runs with epsilon = 1e-14 and maxit = 60 go through it and end with the boundary bit.
GLM_RUNS = [(c, "dominant", "q0", False, 25, 1e-8) for c in ("n40", "n255", "n257", "eq_y")] + \
    [("n257", m, "q2", False, 25, 1e-8) for m in ("additive", "recessive", "genotype")] + \
    [("n255", "genotype", "q0", False, 25, 1e-8), ("n40", "dominant", "q2", True, 25, 1e-8), ("n257", "dominant", "q2", True, 25, 1e-8),
     ("n255", "genotype", "q2", True, 25, 1e-8), ("n257", "dominant", "big", False, 25, 1e-8), ("eq_y", "dominant", "q0", False, 60, 1e-14),
     ("n40", "dominant", "q0", False, 60, 1e-14), ("n257", "dominant", "q0", False, 60, 1e-14), ("n257", "dominant", "q2", True, 60, 1e-14),
     ("n40", "dominant", "sep", False, 60, 1e-14), ("n255", "dominant", "sep", False, 60, 1e-14), ("n257", "genotype", "sep", True, 60, 1e-14),
     ("eq_y", "dominant", "q0", False, 28, 1e-14)]


def glm_reference(run, dtype=np.float64):
    key = ("glm_ref", run, np.dtype(dtype).name)
    if key not in _cache:
        case, model, cov, weighted, maxit, epsilon = run
        c = glm_cohort(case)
        _cache[key] = G.assoc_glm(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], model, c["covar"][cov], c["weight"] if weighted else None,
                                  maxit, epsilon, dtype)
    return _cache[key]


def _floor(v):
    return np.fmax(100.0 * np.where(np.isfinite(v), v, 0.0), 1e-12)


def glm_tolerances(run):
    """Per fit of a run (tol_est [n_fit], tol_dev [n_fit]): 100 x the float64-versus-longdouble difference of the
    restatement for that fit, at least 1e-12 -- est in units of max(|est|, se) and se relative (the larger of the two),
    the deviance relative.  NaN rows (the rank bit) get the floor."""
    return wide_tolerances(glm_reference(run), glm_reference(run, np.longdouble))


# ---- the wide and the terms kernel ------------------------------------------------------------------------------------------
def row(c, name):
    """The allele (= the test, and under every model but ``genotype`` the feature row) of the hard row ``name`` of a cohort."""
    return next(k for k, v in c["names"].items() if v == name)


def glm_sets_of(case):
    """The sets of feature rows (dominant or additive: one row per test) of a wide run, each with what it is for."""
    c = glm_cohort(case)
    lv1 = c["level_rows"][1]
    K = lambda name: row(c, name)                                # noqa: E731
    return [[0, 1, 2],                                           # ordinary
            [1, 2, K("all_cases")],                              # one separated row behind two ordinary ones
            [K("all_controls"), 0, K("quasi")],                  # a separated row first
            [1, lv1],                                            # lv1 - allele 1 = all_cases: a near-zero pivot once W has collapsed there
            [lv1, 1],                                            # the same, the other row dropped
            [K("zero_weight"), 0],                               # weighted: a column of weight 0, pivot exactly 0
            [K("tiny_weight"), 1],                               # weighted: weights 1e-12 on every carrier
            [K("all_cases"), K("all_controls"), K("single_case"), K("quasi"), 0, 1, 2],
            []]                                                  # no row at all: the rank bit


def glm_terms_of(case):
    """The fit records [n_fits, 3, 2] of a terms run."""
    c = glm_cohort(case)
    lv1 = c["level_rows"][1]
    K = lambda name: row(c, name)                                # noqa: E731
    U = (-1, -1)
    return np.array([[(2, -1), (3, -1), (2, 3)],                 # the product is carried by cases only
                     [(2, 3), U, U],                             # the product alone
                     [(1, -1), (K("all_cases"), -1), U],         # a separated main effect
                     [(0, -1), (K("quasi"), -1), (0, K("quasi"))],
                     [(1, -1), (lv1, -1), U],                    # the near-zero pivot of the wide runs
                     [(lv1, -1), U, (1, -1)],
                     [(K("zero_weight"), -1), (0, -1), U],
                     [(K("tiny_weight"), -1), (0, K("tiny_weight")), U],
                     [(0, -1), (1, -1), (0, 1)],                 # ordinary
                     [(K("all_cases"), K("all_controls")), U, U]], np.int32)   # a product nobody carries: the rank bit


# (cohort, model, covariates, weighted, maxit, epsilon) of the wide and of the terms runs.  A run is taken only if its tolerances
# hold the float64 restatement to itself when the samples are merely reordered (tests/test_assoc_hard_host.py): ("n257",
# "additive", "q2") is not -- the fit of [1, lv1] moves by 3.0e-8 in se between sample orders against a tolerance of 1.8e-8 --
# and ("n255", "additive", "q0") with 60 iterations changes its iteration count with the order
WIDE_RUNS = [("n40", "dominant", "q0", False, 25, 1e-8), ("n255", "dominant", "q2", False, 25, 1e-8), ("n255", "additive", "q2", False, 25, 1e-8),
             ("n257", "dominant", "q2", True, 25, 1e-8), ("n255", "dominant", "q0", False, 60, 1e-14), ("n40", "dominant", "q2", True, 60, 1e-14),
             ("n257", "dominant", "sep", False, 60, 1e-14), ("n257", "dominant", "q2", False, 2, 1e-8),
             ("n257", "dominant", "big", False, 25, 1e-8)]


def _wide_reference(kind, run, dtype):
    key = (kind, run, np.dtype(dtype).name)
    if key not in _cache:
        import associnteract_reference as I
        import assocomni_reference as O
        case, model, cov, weighted, maxit, epsilon = run
        c = glm_cohort(case)
        A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], model)
        w = c["weight"] if weighted else None
        if kind == "sets":
            _cache[key] = O.glm_sets(A.F, glm_sets_of(case), c["covar"][cov], w, A.y, maxit, epsilon, dtype)
        else:
            _cache[key] = I.glm_terms(A.F, glm_terms_of(case), c["covar"][cov], w, A.y, maxit, epsilon, dtype)
    return _cache[key]


def sets_reference(run, dtype=np.float64):
    return _wide_reference("sets", run, dtype)


def terms_reference(run, dtype=np.float64):
    return _wide_reference("terms", run, dtype)


def wide_tolerances(r, rl):
    """(tol_est, tol_dev) per fit of a wide or terms run, as ``glm_tolerances``."""
    scale = np.fmax(np.abs(rl["coef"]), rl["se"])
    with np.errstate(invalid="ignore", divide="ignore"):
        g_est = np.nanmax(np.nan_to_num(np.abs(r["coef"] - rl["coef"]) / scale), axis=1)
        g_se = np.nanmax(np.nan_to_num(np.abs(r["se"] / rl["se"] - 1)), axis=1)
        g_dev = np.abs(r["deviance"] / rl["deviance"] - 1)
    return _floor(np.fmax(g_est, g_se)), _floor(g_dev)


# ---- Cox regression ---------------------------------------------------------------------------------------------------------
COX_ROWS = {
    "earliest_k": "the carriers are the four earliest events (the last four events of the time order)",
    "earliest_1": "the one carrier is the earliest event",
    "all_censored": "five carriers, none with an event: a monotone likelihood, the estimate runs to -inf",
    "longest": "the carriers are the four longest follow-ups",
    "tie_block": "the carriers are exactly one tie block with an event and a censored sample in it (n257u: one event)",
}
COX_COVARS = {
    "q0": "no covariates",
    "q2": "two standard normal covariates, centred",
    "mono": "two normal covariates and one that orders the samples as their times do: the base model is monotone",
    "big": "two normal covariates and one of scale 1e3",
    "far": "the two normal covariates, the base model started at (1.7, -1.7), some twenty standard errors from its maximum",
}


def cox_cohort(case):
    """dict a1, a2, event, time (not increasing), n_allele, names, covar (kind -> [q, n], centred), start (kind -> [q] or None)
    of ``case``: "n40", "n255", "n257", "seam" (as many samples as ``S.device_cohort("seam_hi")`` keeps), their times
    rounded to 0.1 and so heavily tied, or "n257u", 257 samples with distinct times: there the single earliest event's first
    Newton step is n = 257, beyond the clamp."""
    if ("cox", case) in _cache:
        return _cache[("cox", case)]
    n = len(S.device_cohort("seam_hi")["time"]) if case == "seam" else int(case[1:4].rstrip("u"))
    rng = np.random.default_rng(n)
    time = np.sort(rng.exponential(1.0, n))[::-1].copy()
    if case != "n257u":
        time = np.round(time, 1)
    event = (rng.random(n) < 0.6).astype(np.int32)
    a = _ordinary(rng, n)
    z = rng.standard_normal((2, n))
    ev = np.flatnonzero(event)
    B = S.Blocks(time)
    free = np.ones(n, bool)
    free[ev[-5:]] = False
    free[:4] = False
    sizes, mixed = np.diff(B.first), np.add.reduceat(event, B.first[:-1])
    ok = [k for k in range(B.nb) if 3 <= sizes[k] <= 8 and 0 < mixed[k] < sizes[k] and free[B.first[k]:B.first[k + 1]].all()]
    block = np.arange(B.first[ok[len(ok) // 2]], B.first[ok[len(ok) // 2] + 1]) if ok else _take(free, event == 1, 1)
    free[block] = False
    plant = [("earliest_k", ev[-4:], 1), ("earliest_1", ev[-1:], 0), ("all_censored", _take(free, event == 0, 5), 1),
             ("longest", np.arange(4), 1), ("tie_block", block, 1)]
    names = {}
    for i, (name, who, slot) in enumerate(plant):
        names[N_ORDINARY + i] = name
        a[who, slot] = N_ORDINARY + i
    mono = -np.arange(n, dtype=np.float64)
    big = 1e3 * rng.standard_normal(n)
    covar = {"q0": np.zeros((0, n)), "q2": S.centred(z), "mono": S.centred(np.vstack([z, mono])), "big": S.centred(np.vstack([z, big])),
             "far": S.centred(z)}
    c = dict(a1=np.ascontiguousarray(a[:, 0]), a2=np.ascontiguousarray(a[:, 1]), event=event, time=time, n_allele=N_ORDINARY + len(plant),
             names=names, covar=covar, start={"far": np.array([1.7, -1.7])})
    _cache[("cox", case)] = c
    return c


# (cohort, model, ties, covariates, maxit)
COX_RUNS = [(c, "dominant", t, q, 20) for c in ("n40", "n255", "n257") for t in S.TIES for q in ("q0", "q2")] + \
    [("seam", "dominant", "efron", "q2", 20), ("seam", "additive", "breslow", "q0", 20), ("n257", "genotype", "efron", "q2", 20),
     ("n255", "dominant", "efron", "mono", 20), ("n40", "dominant", "breslow", "mono", 20), ("n257", "dominant", "efron", "big", 20),
     ("n255", "dominant", "efron", "far", 20), ("n257", "dominant", "efron", "q2", 10), ("n255", "dominant", "efron", "q2", 1),
     ("n257", "dominant", "breslow", "q2", 1), ("n257u", "dominant", "efron", "q0", 1), ("n257u", "dominant", "efron", "q2", 20)]


def cox_reference(run, dtype=np.float64):
    key = ("cox_ref", run, np.dtype(dtype).name)
    if key not in _cache:
        case, model, ties, cov, maxit = run
        c = cox_cohort(case)
        A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, model)
        _cache[key] = S.cox_rows(A.F, model, c["time"], c["covar"][cov], A.y, ties, maxit, 1e-9, dtype, start=c["start"].get(cov))
    return _cache[key]


def cox_tolerances(run):
    """Per fit of a run (tol_est, tol_loglik, tol_score), as ``glm_tolerances``."""
    r, rl = cox_reference(run), cox_reference(run, np.longdouble)
    scale = np.fmax(np.abs(rl["coef"]), rl["se"])
    with np.errstate(invalid="ignore", divide="ignore"):
        g_est = np.nanmax(np.nan_to_num(np.abs(r["coef"] - rl["coef"]) / scale), axis=1)
        g_se = np.nanmax(np.nan_to_num(np.abs(r["se"] / rl["se"] - 1)), axis=1)
        g_ll = np.abs(r["loglik"] / rl["loglik"] - 1)
        g_sc = np.abs(r["score"] / rl["score"] - 1)
    return _floor(np.fmax(g_est, g_se)), _floor(g_ll), _floor(g_sc)


def left_out(tol_est, flags):
    """(mask of the fitted fits whose est and se are left out of the value comparison, number of fitted fits)."""
    fitted = (np.asarray(flags) & 2) == 0
    return fitted & (tol_est > LEFT_OUT_ABOVE), int(fitted.sum())


# ---- the score base fit -----------------------------------------------------------------------------------------------------
# (cohort, covariates, weighted, maxit): the base model y ~ covariates of hlaAssocScore.  Under "sep" it is separated and does
# not converge within maxit, so every test takes the MAXIT failure path (bit 0, no statistic); "q2" is the ordinary base model
# under which the separated rows are tested.
SCORE_RUNS = [("n40", "sep", False, 10), ("n255", "sep", True, 12), ("n257", "q2", True, 25)]


def score_reference(run, dtype=np.float64):
    """The ``assocscore_reference.Score`` of a run with one set per allele row and the wide sets of ``glm_sets_of``
    installed."""
    key = ("score", run, np.dtype(dtype).name)
    if key not in _cache:
        import assocscore_reference as SR
        case, cov, weighted, maxit = run
        c = glm_cohort(case)
        A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], "dominant")
        Z = SR.Score(A.F, A.y, c["covar"][cov], c["weight"] if weighted else None, maxit, 1e-8, dtype)
        _cache[key] = Z.install(score_sets_of(case))
    return _cache[key]


def score_sets_of(case):
    c = glm_cohort(case)
    return [[r] for r in range(c["n_allele"] + 2)] + glm_sets_of(case)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def glm_hla(case):
    """(hla with the prior weights as ``prob``, y, covar [n, 2]) of a logistic cohort, as hlaAssocGlm takes it."""
    c = glm_cohort(case)
    hla, _, _ = AR.hla_of(c["a1"], c["a2"], c["weight"], c["n_allele"])
    return hla, c["y"], c["covar"]["q2"].T


def cox_hla(case):
    """(hla, time, event, covar [n, 2]) of a Cox cohort, the samples shuffled out of time order and the covariates off
    centre, as hlaAssocSurv takes it."""
    c = cox_cohort(case)
    p = np.random.default_rng(5).permutation(len(c["time"]))
    hla, _, _ = AR.hla_of(c["a1"][p], c["a2"][p], None, c["n_allele"])
    return hla, c["time"][p], c["event"][p], (c["covar"]["q2"] + 3.0)[:, p].T


def score_base_tolerance(run):
    """100 x the float64-versus-longdouble difference of the base fit (est in units of max(|est|, se), se and deviance
    relative), at least 1e-12."""
    b, bl = score_reference(run).base, score_reference(run, np.longdouble).base
    scale = np.fmax(np.abs(bl["coef"]), bl["se"])
    gap = max(np.max(np.abs(b["coef"] - bl["coef"]) / scale), np.max(np.abs(b["se"] / bl["se"] - 1)), abs(b["deviance"] / bl["deviance"] - 1))
    return max(100.0 * float(gap), 1e-12)
