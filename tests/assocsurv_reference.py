"""CPU restatement of hlaAssocSurv for the tests: DESIGN.md section 31 items 1-7 in numpy, written from the definitions.

The Efron / Breslow score and information with the order of summation swapped.  With ``r_j = exp(x_j beta)``, the usual
forms are ``U = sum_events x_j - sum_k sum_l (S1_k - f D1_k) / phi_kl`` and
``I = sum_k sum_l [(S2_k - f D2_k) / phi_kl - v_kl v_kl']``, where ``S2_k = sum_{b(j) <= k} r_j x_j x_j'`` and ``D2_k`` the same
over the events of block k.  Collecting the coefficient of ``r_j x_j x_j'`` (and of ``r_j x_j``) over all (k, l) gives
``sum_{k >= b(j)} a_k - e_j b_b(j) = A_b(j) - e_j b_b(j) = w_j / r_j``: so ``sum_k sum_l (S2_k - f D2_k) / phi_kl =
sum_j w_j x_j x_j'`` and ``sum_k sum_l v_kl = sum_j w_j x_j``, and no p x p matrix is kept per event time.

Dtype-generic like tests/assocglm_reference.py, whose Cholesky factorisation and solves it uses: ``evaluate`` is item 4,
``fit`` items 5-6, ``cox_rows`` what ``hibag_hip_assoc_cox`` returns (the base model first), ``Backend`` the same behind the
interface ``hibag_amd.assocsurv`` drives, so that ``hlaAssocSurv`` itself runs on the restatement."""

from __future__ import annotations

import numpy as np

import assoc_reference as AR
import assocglm_reference as G
from assoc_reference import allele_names, kept_columns       # noqa: F401  (the tests reach them through this module)

MODELS = AR.MODELS
SLOTS, COV0, MAX_COVAR = 16, 2, 12
MAXIT_BIT, RANK_BIT, CLAMP_BIT, DECREASE_BIT = 1, 2, 4, 8
TIES = ("efron", "breslow")
ETA_MAX = 200


class Blocks:
    """The block table of times in descending order (item 1): ``first`` [nb + 1] the first sample of every block
    (first[nb] = n), ``blk`` [n] the block of a sample."""

    def __init__(self, time):
        time = np.asarray(time, np.float64)
        assert (np.diff(time) <= 0).all(), "the samples come in time order, latest first"
        n = len(time)
        new = np.r_[True, time[1:] != time[:-1]] if n else np.zeros(0, bool)
        self.first = np.r_[np.flatnonzero(new), n]
        self.blk = np.cumsum(new) - 1
        self.last = self.first[1:] - 1
        self.nb = len(self.last)


def evaluate(X, e, B, beta, ties="efron", dtype=np.float64):
    """Item 4 at beta: (loglik, U [p], I [p, p], clamped, diag G [p]) with G = sum w x x', the Gram I = G - V is left of."""
    X = np.asarray(X, dtype)
    n, p = X.shape
    ev = np.asarray(e) != 0
    eta = X @ np.asarray(beta, dtype) if p else np.zeros(n, dtype)
    clamped = bool((np.abs(eta) > ETA_MAX).any())
    eta = np.clip(eta, dtype(-ETA_MAX), dtype(ETA_MAX))
    r = np.exp(eta)
    rx = r[:, None] * X
    starts = B.first[:-1]
    S0, S1 = np.cumsum(r)[B.last], np.cumsum(rx, axis=0)[B.last]
    D0, D1 = np.add.reduceat(np.where(ev, r, dtype(0)), starts), np.add.reduceat(np.where(ev[:, None], rx, dtype(0)), starts, axis=0)
    d = np.add.reduceat(ev.astype(np.int64), starts)
    kk = np.flatnonzero(d > 0)                                   # the blocks with events; one (k, l) pair per event
    pk = np.repeat(kk, d[kk])
    pstart = np.r_[0, np.cumsum(d[kk])[:-1]]
    l = np.arange(len(pk)) - np.repeat(pstart, d[kk])
    f = (l.astype(dtype) / d[pk].astype(dtype)) if ties == "efron" else np.zeros(len(pk), dtype)
    phi = S0[pk] - f * D0[pk]
    v = (S1[pk] - f[:, None] * D1[pk]) / phi[:, None]
    a, b = np.zeros(B.nb, dtype), np.zeros(B.nb, dtype)
    if len(kk):
        a[kk] = np.add.reduceat(1 / phi, pstart)
        b[kk] = np.add.reduceat(f / phi, pstart)
    A = np.cumsum(a[::-1])[::-1]
    w = r * (A[B.blk] - np.where(ev, b[B.blk], dtype(0)))
    loglik = np.where(ev, eta, dtype(0)).sum() - np.log(phi).sum()
    U = np.where(ev[:, None], X, dtype(0)).sum(axis=0) - (w[:, None] * X).sum(axis=0)
    gram = X.T @ (w[:, None] * X)
    return loglik, U, gram - v.T @ v, clamped, np.diag(gram)


def inverse_block(L, d, dtype):
    """The leading d x d block of (L L')^-1: the dot products of the first d columns of L^-1."""
    p = len(L)
    cols = []
    for j in range(d):
        x = np.zeros(p, dtype)
        for i in range(j, p):
            v = dtype(1) if i == j else dtype(0)
            for m in range(j, i):
                v = v - L[i, m] * x[m]
            x[i] = v / L[i, i]
        cols.append(x)
    return np.array([[(cols[i] * cols[j]).sum() for j in range(d)] for i in range(d)], dtype).reshape(d, d)


def fit(X, e, B, start, d, ties="efron", maxit=20, epsilon=1e-9, dtype=np.float64):
    """One fit of items 5-6 from ``start``; the first ``d`` columns of X are the h columns.  dict coef, se [p], loglik,
    score, iterations, flags, crit (every iteration's), pivots (every tested pivot with its threshold)."""
    p = X.shape[1]
    nan = np.full(p, np.nan)
    beta = np.asarray(start, dtype).copy()
    ll, U, info, clamped, gdiag = evaluate(X, e, B, beta, ties, dtype)
    flags = CLAMP_BIT if clamped else 0
    if p == 0:
        return dict(coef=nan, se=nan, loglik=ll, score=np.nan, iterations=0, flags=flags, crit=[], pivots=[])
    score, crits, pivots, L = np.nan, [], [], None
    for k in range(1, maxit + 1):
        L = G.cholesky(info, dtype, scale=gdiag, pivots=pivots)          # a pivot is judged against G_jj (item 5)
        if L is None:
            return dict(coef=nan, se=nan, loglik=np.nan, score=np.nan, iterations=k, flags=RANK_BIT, crit=crits, pivots=pivots)
        if k == 1 and d > 0:
            M = inverse_block(L, d, dtype)
            score = sum(U[i] * M[i, j] * U[j] for i in range(d) for j in range(d))
        beta = beta + G.solve(L, U, dtype)
        ll_new, U, info, clamped, gdiag = evaluate(X, e, B, beta, ties, dtype)
        if clamped:
            flags |= CLAMP_BIT
        with np.errstate(divide="ignore", invalid="ignore"):
            crit = abs(1 - ll / ll_new)
        crits.append(float(crit))
        decreased, ll = ll_new < ll, ll_new
        if crit <= epsilon:
            break
        if decreased:                                            # (a decrease within epsilon is convergence)
            flags |= DECREASE_BIT
    else:
        flags |= MAXIT_BIT
    return dict(coef=beta, se=np.sqrt(G.inverse_diagonal(L, dtype)), loglik=ll, score=score, iterations=k, flags=flags, crit=crits,
                pivots=pivots)


def fit_slots(rsum, model, n):
    """Per test the feature rows behind slots 0 and 1 (-1: unused), or None for a test that is not fitted (item 7)."""
    return G.fit_slots(None, rsum, model, n)


def cox_rows(F, model, time, covar, e, ties="efron", maxit=20, epsilon=1e-9, dtype=np.float64, start=None):
    """What hibag_hip_assoc_cox returns from the feature rows F [rows, n] in time order: dict of coef, se [1 + T, 16] by
    slot (float64), loglik, score, iterations, flags [1 + T], and crit and pivots, lists of every fit's criteria and tested pivots; fit 0 is the base
    model.  covar [q, n] is taken as it is (the caller centres it)."""
    n = F.shape[1]
    covar = np.zeros((0, n)) if covar is None else np.asarray(covar, np.float64).reshape(-1, n)
    q = len(covar)
    assert q <= MAX_COVAR
    B = Blocks(time)
    e = np.asarray(e)
    slots = [(-1, -1)] + fit_slots(F.sum(axis=1), model, n)
    if not (e != 0).any():
        slots = [None] * len(slots)
    n_fit = len(slots)
    out = dict(coef=np.full((n_fit, SLOTS), np.nan), se=np.full((n_fit, SLOTS), np.nan), loglik=np.full(n_fit, np.nan),
               score=np.full(n_fit, np.nan), iterations=np.zeros(n_fit, np.int32), flags=np.zeros(n_fit, np.int32),
               crit=[[] for _ in range(n_fit)], pivots=[[] for _ in range(n_fit)])
    base = np.zeros(q) if start is None else np.asarray(start, np.float64)
    for f, rows in enumerate(slots):
        if rows is None:
            out["flags"][f] = RANK_BIT
            continue
        hs = [r for r in rows if r >= 0]
        used = [i for i, r in enumerate(rows) if r >= 0] + list(range(COV0, COV0 + q))
        X = np.stack([F[r].astype(np.float64) for r in hs] + list(covar), axis=1) if used else np.zeros((n, 0))
        res = fit(X, e, B, np.r_[np.zeros(len(hs)), base], len(hs), ties, maxit, epsilon, dtype)
        out["coef"][f, used] = np.asarray(res["coef"], np.float64)
        out["se"][f, used] = np.asarray(res["se"], np.float64)
        out["loglik"][f], out["score"][f] = float(res["loglik"]), float(res["score"])
        out["iterations"][f], out["flags"][f], out["crit"][f] = res["iterations"], res["flags"], res["crit"]
        out["pivots"][f] = res["pivots"]
        if f == 0:
            if res["flags"] & RANK_BIT:                          # no base model, no start: every test is reported like it
                out["flags"][1:] = RANK_BIT
                break
            base = np.asarray(res["coef"], np.float64) if q else base
    return out


def sort_cohort(a1, a2, time, event, *columns):
    """The cohort's samples with two known alleles in the order of item 1 (time descending, stable): (a1, a2, time, event,
    columns restricted and ordered alike), as hlaAssocSurv hands them to the handle."""
    a1, a2, time, event = np.asarray(a1), np.asarray(a2), np.asarray(time, np.float64), np.asarray(event)
    keep = np.flatnonzero((a1 != AR.NA_INTEGER) & (a2 != AR.NA_INTEGER))
    o = keep[np.argsort(-time[keep], kind="stable")]
    return (np.ascontiguousarray(a1[o]), np.ascontiguousarray(a2[o]), np.ascontiguousarray(time[o]),
            np.ascontiguousarray(event[o]).astype(np.int32)) + tuple(np.ascontiguousarray(np.asarray(c)[..., o]) for c in columns)


def centred(covar):
    covar = np.asarray(covar, np.float64)
    return covar - covar.mean(axis=1, keepdims=True) if covar.size else covar


class Backend(AR.Backend):
    """The restatement behind the interface of hibag_amd.assocsurv._DeviceSurv (``hlaAssocSurv(..., _backend=Backend)``)."""

    def cox(self, time, covar, ties, maxit, epsilon):
        r = cox_rows(self.A.F, self.model, time, covar, self.A.y, TIES[ties], maxit, epsilon, self.dtype)
        type(self).last = r
        return r["coef"], r["se"], r["loglik"], r["score"], r["iterations"], r["flags"]


# ---- the cohorts of the tests ---------------------------------------------------------------------------------------
def cohort(n, n_allele, q, seed, partition=False, ties=None, censor=0.3):
    """(a1, a2, time, event, group_of or None, covar [q, n]): alleles drawn from frequencies ~ 0.75^k, exponential times with
    the effects of alleles 0 and 1 and of the covariates, independent exponential censoring of about ``censor``, three
    samples with an unknown allele.  ``ties``: None (all times distinct) or the number of distinct values the times are
    rounded to."""
    rng = np.random.default_rng(seed)
    w = 0.75 ** np.arange(n_allele)
    a = rng.choice(n_allele, (n, 2), p=w / w.sum()).astype(np.int32)
    covar = rng.standard_normal((q, n))
    gamma = rng.uniform(-0.5, 0.5, q) / np.sqrt(max(q, 1))
    eta = 0.7 * (a == 0).any(axis=1) - 0.6 * (a == 1).any(axis=1) + gamma @ covar
    t_event = rng.exponential(1.0, n) / np.exp(eta)
    t_cens = rng.exponential((1 - censor) / censor, n)
    time, event = np.minimum(t_event, t_cens), (t_event <= t_cens).astype(np.int32)
    if ties is not None:
        time = np.ceil(time / time.max() * ties)
    a[rng.choice(n, 3, replace=False), rng.integers(0, 2, 3)] = AR.NA_INTEGER
    g = AR.gap_partition(n_allele) if partition else None
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), time, event, g, covar


def analysis(a1, a2, time, event, n_allele, group_of, model, covar):
    """(Analysis in time order, time, centred covar) of a cohort."""
    a1, a2, time, event, covar = sort_cohort(a1, a2, time, event, covar)
    return AR.Analysis(a1, a2, event, n_allele, group_of, model), time, centred(covar)


def cox_cohort(a1, a2, time, event, n_allele, group_of, model, covar, ties="efron", maxit=20, epsilon=1e-9, dtype=np.float64):
    A, time, covar = analysis(a1, a2, time, event, n_allele, group_of, model, covar)
    return cox_rows(A.F, model, time, covar, A.y, ties, maxit, epsilon, dtype)


def gaps(r, rl):
    """The largest differences of two results over the fits without the rank bit: est in units of max(|est|, se); se, loglik
    and score relative."""
    ok = (rl["flags"] & RANK_BIT) == 0
    if not ok.any():
        return 0.0, 0.0, 0.0, 0.0
    scale = np.fmax(np.abs(rl["coef"]), rl["se"])
    with np.errstate(invalid="ignore", divide="ignore"):
        g_est = np.abs(r["coef"] - rl["coef"])[ok] / scale[ok]
        g_se = np.abs(r["se"] / rl["se"] - 1)[ok]
        g_ll = np.abs(r["loglik"] / rl["loglik"] - 1)[ok]
        g_sc = np.abs(r["score"] / rl["score"] - 1)[ok]
    return tuple(float(np.nanmax(v)) if np.isfinite(v).any() else 0.0 for v in (g_est, g_se, g_ll, g_sc))


# (samples, alleles, covariates, seed, with a partition whose level 1 is empty, the times' ties): ``seam_lo`` / ``seam_hi``
# have their last kept sample one matrix-core step below / above a seam between two waves' segments and a tie block across
# every seam (the constants come from hibag_hip_assoc_cox_segment); ``n1000`` has one block of more than 64 events
CASES = {"n6": None, "n40": (40, 6, 0, 1, False, None), "n255": (255, 12, 1, 2, False, 10), "n256": (256, 12, 5, 3, False, 10),
         "n257": (257, 12, 12, 4, False, 10), "seam_lo": (None, 12, 5, 6, False, "seams"), "seam_hi": (None, 12, 5, 7, False, "seams"),
         "n1000": (1000, 20, 6, 5, True, "big"), "one_time": (60, 6, 1, 8, False, "one"), "late_censored": (60, 6, 1, 9, False, "late"),
         "one_event": (60, 6, 1, 10, False, "single")}
SEAM = 7                                                         # the seam the seam cases end next to
COX_WAVES = 8                                                    # the segments of a fit (COX_WAVES of hibag_k_cox.h)


def segment_of(n_kept):
    """(samples per matrix-core step, samples per wave segment) of the device's walk at n_kept samples, from the library (a
    host function: no device is needed)."""
    import ctypes as C
    from hibag_amd import _lib
    step, seg = C.c_int(), C.c_int()
    _lib.check(_lib.lib().hibag_hip_assoc_cox_segment(int(n_kept), C.byref(step), C.byref(seg)))
    return step.value, seg.value


_COHORTS = {}


def device_cohort(case):
    """The case as the handle takes it: dict a1, a2 (all samples, in time order, three with an unknown allele), event, g,
    n_allele and, over the kept samples, time (not increasing) and covar [q, n_kept] centred.  Computed once; callers do not
    modify it."""
    if case in _COHORTS:
        return _COHORTS[case]
    if case == "n6":                                             # the six-subject example: allele 0 is x
        time, status, x = np.array([1, 1, 6, 6, 8, 9.0]), np.array([1, 0, 1, 1, 0, 1]), np.array([1, 1, 1, 0, 0, 0])
        o = np.argsort(-time, kind="stable")
        c = dict(a1=(1 - x[o]).astype(np.int32), a2=np.ones(6, np.int32), event=status[o].astype(np.int32), g=None, n_allele=2,
                 time=time[o], covar=np.zeros((0, 6)))
        _COHORTS[case] = c
        return c
    n, n_allele, q, seed, partition, kind = CASES[case]
    step = seg = None
    if kind == "seams":
        step, seg = segment_of(400)                              # 385 .. 512 kept samples share their segment size
        n = SEAM * seg + (-step if case == "seam_lo" else step) + 3
        assert segment_of(n - 3) == (step, seg)
    a1, a2, time, event, g, covar = cohort(n, n_allele, q, seed, partition, ties=10 if kind == 10 else None)
    o = np.argsort(-time, kind="stable")
    a1, a2, time, event, covar = a1[o], a2[o], time[o], event[o], covar[:, o]
    keep = np.flatnonzero((a1 != AR.NA_INTEGER) & (a2 != AR.NA_INTEGER))
    tk, ek = time[keep].copy(), event[keep].copy()
    if kind == "seams":
        for w in range(1, COX_WAVES):
            if w * seg + 3 <= len(tk):
                tk[w * seg - 3:w * seg + 3] = tk[w * seg - 3]
                ek[w * seg - 2:w * seg + 2] = 1                  # events on both sides of the seam
    elif kind == "big":
        tk[300:400] = tk[300]
        assert ek[300:400].sum() > 64
    elif kind == "one":
        tk[:] = 2.0
    elif kind == "late":
        ek[:15] = 0                                              # the fifteen longest follow-ups are censored
    elif kind == "single":
        ek[:] = 0
        ek[20] = 1
    event = event.copy()
    event[keep] = ek
    c = dict(a1=np.ascontiguousarray(a1), a2=np.ascontiguousarray(a2), event=event.astype(np.int32), g=g, n_allele=n_allele,
             time=np.ascontiguousarray(tk), covar=centred(covar[:, keep]), step=step, segment=seg)
    _COHORTS[case] = c
    return c


_CACHE = {}


def reference(case, model, ties="efron", maxit=20, dtype=np.float64, alleles_only=False):
    """cox_rows of a case, computed once per process and shared (callers do not modify it)."""
    key = (case, model, ties, maxit, np.dtype(dtype).name, alleles_only)
    if key not in _CACHE:
        c = device_cohort(case)
        A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None if alleles_only else c["g"], model)
        _CACHE[key] = cox_rows(A.F, model, c["time"], c["covar"], A.y, ties, maxit, 1e-9, dtype)
    return _CACHE[key]


# every (case, model, ties, maxit) whose fits tests/test_hip_assocsurv.py compares with the device; tests/test_assocsurv_host.py
# asserts the safety condition (no convergence criterion within 1e-6 relative of epsilon) for each of them
DEVICE_RUNS = [(case, model, ties, 20) for case in CASES for model in MODELS for ties in TIES] + \
    [("n257", model, "efron", 2) for model in MODELS]


def tolerance(case, model, ties="efron", maxit=20):
    """100 x the largest float64-versus-longdouble difference of the restatement over the run's fits without the rank bit
    (est in units of max(|est|, se); se, loglik and score relative), at least 1e-12."""
    r, rl = reference(case, model, ties, maxit), reference(case, model, ties, maxit, np.longdouble)
    assert np.array_equal(r["flags"], rl["flags"]) and np.array_equal(r["iterations"], rl["iterations"]), (case, model, ties)
    return max(100.0 * max(gaps(r, rl)), 1e-12)


def hla_of(case):
    """A case's cohort as hlaAssocSurv takes it, the samples shuffled out of time order: (hla, time, event, groups or None,
    covar [n, q])."""
    c = device_cohort(case)
    n = len(c["a1"])
    keep = np.flatnonzero((c["a1"] != AR.NA_INTEGER) & (c["a2"] != AR.NA_INTEGER))
    time = np.full(n, 1.0)
    time[keep] = c["time"]
    rng = np.random.default_rng(99)
    covar = rng.standard_normal((c["covar"].shape[0], n))
    covar[:, keep] = c["covar"] + 3.0                            # (off centre: hlaAssocSurv centres)
    p = rng.permutation(n)
    hla, _, groups = AR.hla_of(c["a1"][p], c["a2"][p], None, c["n_allele"], c["g"])
    return hla, time[p], c["event"][p], groups, covar[:, p].T
