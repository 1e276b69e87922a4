"""The hard cohorts of tests/assoc_hard_corpus.py on the host: the restatements alone prove that the
corpus is what it claims to be -- every planted row has the carriers its name says, every branch written for a hard case is
reached by a fit that the device tests compare -- and assert the safety conditions of tests/test_hip_assoc_hard.py: the
float64 and the longdouble restatement agree on flags, iterations and dropped columns of every compared fit, no convergence
criterion lies within 1e-6 relative of epsilon, no pivot within 1e-3 relative of its threshold, at most a quarter of a run's
fits have est and se left out of the value comparison, no Cox fit without the rank bit reports a runaway coefficient, and
the float64 restatement with its samples reordered (Cox: inside the tie blocks) stays within a quarter of every tolerance.  The
quasi-separated rows, which have a finite maximum, are compared with the independent scipy.optimize maxima of
tests/test_assocglm_host.py and tests/test_assocsurv_host.py."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_hard_corpus as H  # noqa: E402
import assoc_reference as AR  # noqa: E402
import assocglm_reference as G  # noqa: E402
import assocomni_reference as O  # noqa: E402
import assocsurv_reference as S  # noqa: E402
from test_assocglm_host import EST_BOUND, SE_BOUND, _gap  # noqa: E402
from test_assocglm_host import _mle as glm_mle  # noqa: E402
from test_assocsurv_host import _mle as cox_mle  # noqa: E402

import hibag_amd as hb  # noqa: E402

# A pivot d = A_jj - sum L^2 near its threshold 1e-11 A_jj is what a cancellation of eleven digits leaves: it carries a
# relative rounding error near 2^-53 / 1e-11 = 1e-5, so the margin asked of a pivot is 1e-3, not the 1e-6 of a criterion.
PIVOT_MARGIN = 1e-3
CRIT_MARGIN = 1e-6
# No Cox fit without the rank bit may report a beta with |x_j beta| beyond twice the clamp for any sample.  Every evaluation
# clamps eta to [-200, 200], so a beta inside 2 x 200 is at most one step of the size of the whole clamped range past an
# evaluation that was inside it; the largest honest first step of the corpus is the single earliest event's among n untied
# samples, U / I = (1 - 1/n) / ((1/n)(1 - 1/n)) = n = 257.  A step from an information that cancellation has emptied is 1e88.
ETA_BOUND = 2 * S.ETA_MAX

ids = lambda run: "-".join(str(v) for v in run)                  # noqa: E731


_row = H.row


# 1 the corpus is what it claims --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n40", "n255", "n257"])
def test_logistic_cohorts(case):
    c = H.glm_cohort(case)
    n = len(c["y"])
    assert n == int(case[1:]) and set(c["names"].values()) <= set(H.GLM_ROWS) and c["n_allele"] == H.N_ORDINARY + len(c["names"])
    A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], "genotype")
    assert A.n == n
    het, hom, y = A.F[0::2], A.F[1::2], A.y
    car = (het + hom) > 0
    k = 4 if n == 40 else 6
    assert car[_row(c, "all_cases")].sum() == k and y[car[_row(c, "all_cases")]].all()
    assert car[_row(c, "all_controls")].sum() == k and not y[car[_row(c, "all_controls")]].any()
    assert car[_row(c, "single_case")].sum() == 1 and y[car[_row(c, "single_case")]].all()
    q = car[_row(c, "quasi")]
    assert q.sum() == 6 and y[q].sum() == 5
    zw, tw = car[_row(c, "zero_weight")], car[_row(c, "tiny_weight")]
    assert zw.sum() == 3 and (c["weight"][zw] == 0).all() and (c["weight"][~zw] > 0).all()
    assert tw.sum() == 4 and (c["weight"][tw] == 1e-12).all() and y[tw].sum() == 2
    if n > 40:
        r = _row(c, "het_sep")
        assert het[r].sum() == 6 and y[het[r] > 0].all() and hom[r].sum() == 4 and y[hom[r] > 0].sum() == 2
        r = _row(c, "hom_sep")
        assert het[r].sum() == 6 and y[het[r] > 0].sum() == 3 and hom[r].sum() == 3 and y[hom[r] > 0].all()
    both = car[2] & car[3]
    assert both.sum() >= 3 and y[both].all()                     # the interaction product is carried by cases only
    lv0, lv1 = c["level_rows"]
    apart = car[lv1] & ~car[1]                                   # the two rows differ on separated samples only
    assert np.array_equal(car[lv1], car[1] | car[_row(c, "all_cases")]) and apart.sum() >= 2 and y[apart].all()
    for r in range(H.N_ORDINARY):                                # the ordinary alleles have cases and controls on either side
        assert 0 < y[car[r]].sum() < car[r].sum() and 0 < y[~car[r]].sum() < (~car[r]).sum()
    assert set(c["covar"]) == set(H.GLM_COVARS)
    sep, big = c["covar"]["sep"][2], c["covar"]["big"][2]
    assert sep[y == 1].min() >= 1 and sep[y == 0].max() <= -1 and 500 < big.std() < 2000


def test_the_feature_equal_to_y():
    c = H.glm_cohort("eq_y")
    A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], None, "dominant")
    assert np.array_equal(A.F[H.N_ORDINARY], A.y) and 5 < A.y.sum() < 35


@pytest.mark.parametrize("case", ["n40", "n255", "n257", "seam", "n257u"])
def test_cox_cohorts(case):
    c = H.cox_cohort(case)
    n = len(c["time"])
    assert n == {"n40": 40, "n255": 255, "n257": 257, "n257u": 257, "seam": len(S.device_cohort("seam_hi")["time"])}[case]
    assert (np.diff(c["time"]) <= 0).all() and set(c["names"].values()) == set(H.COX_ROWS)
    A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, "dominant")
    car, e = A.F > 0, A.y
    ev = np.flatnonzero(e)
    assert np.array_equal(np.flatnonzero(car[_row(c, "earliest_k")]), ev[-4:])
    assert np.array_equal(np.flatnonzero(car[_row(c, "earliest_1")]), ev[-1:])
    assert car[_row(c, "all_censored")].sum() == 5 and not e[car[_row(c, "all_censored")]].any()
    assert np.array_equal(np.flatnonzero(car[_row(c, "longest")]), np.arange(4))
    B = S.Blocks(c["time"])
    tb = np.flatnonzero(car[_row(c, "tie_block")])
    assert B.blk[tb[0]] == B.blk[tb[-1]] and len(tb) == B.first[B.blk[tb[0]] + 1] - B.first[B.blk[tb[0]]] and e[tb].any()
    if case == "n257u":
        assert B.nb == n
    else:
        assert B.nb <= n / 2 and 3 <= len(tb) <= 8 and not e[tb].all()
    assert set(c["covar"]) == set(H.COX_COVARS)
    for k, cov in c["covar"].items():
        assert np.abs(cov.mean(axis=1)).max(initial=0.0) < 1e-9 * max(1.0, np.abs(cov).max(initial=0.0)), k
    mono = c["covar"]["mono"][2]
    assert (np.diff(mono) < 0).all() and 500 < c["covar"]["big"][2].std() < 2000


# 2 every branch is reached by a compared fit -----------------------------------------------------------------------------
def test_every_glm_branch_is_reached():
    """Per kernel: the boundary bit, |eta| > 30 in an iteration's weights, maxit on a diverging fit, the rank bit from a column
    of weight 0 (its first pivot is exactly 0), and for the wide and the terms kernel a column dropped on a pivot that is small
    but not 0."""
    flags, eta = 0, 0.0
    for run in H.GLM_RUNS:
        r, c = H.glm_reference(run), H.glm_cohort(run[0])
        flags |= int(np.bitwise_or.reduce(r["flags"]))
        eta = max(eta, max(r["eta_max"]))
        if run[3]:                                               # weighted: the zero-weight row fails at its first factorisation
            f = _row(c, "zero_weight")
            assert r["flags"][f] == G.RANK_BIT and r["iterations"][f] == 1 and r["pivots"][f][-1] == (0.0, 0.0)
            assert r["flags"][_row(c, "tiny_weight")] & G.RANK_BIT == 0
    assert flags == G.MAXIT_BIT | G.RANK_BIT | G.BOUNDARY_BIT and eta > 30
    # the rank bit late in a fit, on a pivot that is small but not 0: a level of the partition (eq_y: level 1, n40: level 0)
    # whose row is told from the intercept by separated samples alone, once their weights have collapsed
    for run, lv, it in ((("eq_y", "dominant", "q0", False, 60, 1e-14), 1, 25), (("n40", "dominant", "q0", False, 60, 1e-14), 0, 24)):
        r, f = H.glm_reference(run), H.glm_cohort(run[0])["level_rows"][lv]
        d, limit = r["pivots"][f][-1]
        assert r["flags"][f] == G.RANK_BIT and r["iterations"][f] == it and 0.5 * limit < d < 0.9 * limit, (run, r["iterations"][f], d, limit)
    r = H.glm_reference(("eq_y", "dominant", "q0", False, 28, 1e-14))
    assert r["flags"][H.N_ORDINARY] == G.MAXIT_BIT and abs(r["coef"][H.N_ORDINARY, 1]) > 50        # maxit on a diverging fit
    for ref in (H.sets_reference, H.terms_reference):
        flags, small = 0, 0
        for run in H.WIDE_RUNS:
            r = ref(run)
            flags |= int(np.bitwise_or.reduce(r["flags"]))
            small += sum(1 for f, rr in enumerate(r["ratios"]) if r["flags"][f] & O.ALIASED_BIT and any(0 < v <= 1e-11 for v in rr))
        assert flags == O.MAXIT_BIT | O.RANK_BIT | O.BOUNDARY_BIT | O.ALIASED_BIT and small >= 2, (flags, small)
    for run in H.SCORE_RUNS:
        Z = H.score_reference(run)
        if run[1] == "sep":                                      # the failure path: bit 0 on every test, no statistic
            assert Z.base["flags"] & G.MAXIT_BIT and (Z.flags & 1).all() and (Z.df == 0).all() and np.isnan(np.asarray(Z.stat, float)).all()
        else:
            assert Z.base["flags"] == 0 and (Z.flags & 1 == 0).all() and (Z.df > 0).sum() > 15


def test_default_controls_stop_before_the_boundary():
    """With maxit = 25 and epsilon = 1e-8 a separated fit converges near |eta| = 16 (the feature equal to y: runs into maxit
    near 26): neither the |eta| > 30 substitution nor the boundary bit is reached unless the covariates separate y."""
    seen = 0
    for run in H.GLM_RUNS:
        if run[4:] == (25, 1e-8):
            r = H.glm_reference(run)
            assert max(r["eta_max"]) < 30 and not (r["flags"] & G.BOUNDARY_BIT).any(), run
            assert max(r["eta_max"]) > 13                        # (and yet the fit is separated)
            seen += 1
    assert seen >= 8


def test_every_cox_branch_is_reached():
    flags = 0
    for run in H.COX_RUNS:
        r = H.cox_reference(run)
        flags |= int(np.bitwise_or.reduce(r["flags"]))
    assert flags == S.MAXIT_BIT | S.RANK_BIT | S.CLAMP_BIT | S.DECREASE_BIT
    # the clamp: the single earliest event among 257 untied samples, whose first step is n - 1
    c = H.cox_cohort("n257u")
    r = H.cox_reference(("n257u", "dominant", "efron", "q0", 1))
    f = 1 + _row(c, "earliest_1")
    assert r["flags"][f] == S.MAXIT_BIT | S.CLAMP_BIT and abs(r["coef"][f, 0] - 256) < 1e-9
    # a decrease that the fit recovers from: the base model from the far start
    r = H.cox_reference(("n255", "dominant", "efron", "far", 20))
    assert r["flags"][0] == S.DECREASE_BIT and np.allclose(r["coef"][0, 2:4], H.cox_reference(("n255", "dominant", "efron", "q2", 20))["coef"][0, 2:4],
                                                            rtol=1e-6)
    # maxit on a diverging fit: carriers without an event
    c = H.cox_cohort("n257")
    r = H.cox_reference(("n257", "dominant", "efron", "q2", 10))
    f = 1 + _row(c, "all_censored")
    assert r["flags"][f] == S.MAXIT_BIT and r["coef"][f, 0] < -8


def test_a_collapsed_information_has_the_rank_bit():
    """The carriers are the earliest events: the first step overshoots, r = exp(eta) of the carriers dominates every risk set
    and I = G - V is what the cancellation leaves.  Judged against G_jj it fails in either precision, in the second or a
    later iteration, where the rule 1e-11 I_jj compared the remainder with itself."""
    seen = 0
    for run in H.COX_RUNS:
        if run[4] < 20 or run[3] == "mono":                      # (the monotone covariate takes the earliest events' risk up itself)
            continue
        c = H.cox_cohort(run[0])
        for dtype in (np.float64, np.longdouble):
            r = H.cox_reference(run, dtype)
            for name in ("earliest_k", "earliest_1"):
                f = 1 + _row(c, name)
                d, limit = r["pivots"][f][-1]
                assert r["flags"][f] == S.RANK_BIT and r["iterations"][f] >= 2 and d <= limit and np.isnan(r["coef"][f]).all(), (run, name)
                seen += 1
    assert seen >= 40


# 3 the safety conditions of the device tests -----------------------------------------------------------------------------
def _same(r, rl, keys):
    return all(np.array_equal(r[k], rl[k]) for k in keys) and np.array_equal(np.isnan(r["coef"]), np.isnan(rl["coef"]))


def _criteria_clear(r, epsilon, run):
    for f, crits in enumerate(r["crit"]):
        for c in crits:
            assert abs(c - epsilon) > CRIT_MARGIN * epsilon, (run, f, c)


def _quarter(tol_est, flags, run):
    out, fitted = H.left_out(tol_est, flags)
    assert 4 * int(out.sum()) <= fitted, (run, int(out.sum()), fitted)
    return int(out.sum()), fitted


@pytest.mark.parametrize("run", H.GLM_RUNS, ids=ids)
def test_glm_runs_do_not_depend_on_rounding(run):
    r, rl = H.glm_reference(run), H.glm_reference(run, np.longdouble)
    assert _same(r, rl, ("flags", "iterations")), (r["flags"], rl["flags"], r["iterations"], rl["iterations"])
    _criteria_clear(r, run[5], run)
    for f, pv in enumerate(r["pivots"]):
        for d, limit in pv:
            assert (d == 0 and limit == 0) or abs(d - limit) > PIVOT_MARGIN * limit, (run, f, d, limit)
    out, fitted = _quarter(H.glm_tolerances(run)[0], r["flags"], run)
    print(f"{ids(run)}: {out} of {fitted} fits have est and se left out")


@pytest.mark.parametrize("kind", ["sets", "terms"])
@pytest.mark.parametrize("run", H.WIDE_RUNS, ids=ids)
def test_wide_runs_do_not_depend_on_rounding(run, kind):
    ref = H.sets_reference if kind == "sets" else H.terms_reference
    r, rl = ref(run), ref(run, np.longdouble)
    assert _same(r, rl, ("flags", "iterations", "df_h")), (r["flags"], rl["flags"], r["iterations"], rl["iterations"])
    _criteria_clear(r, run[5], run)
    for f, rr in enumerate(r["ratios"]):
        for v in rr:
            assert abs(v - 1e-11) > PIVOT_MARGIN * 1e-11, (run, f, v)
    out, fitted = _quarter(H.wide_tolerances(r, rl)[0], r["flags"], run)
    print(f"{kind} {ids(run)}: {out} of {fitted} fits have est and se left out")


@pytest.mark.parametrize("run", H.COX_RUNS, ids=ids)
def test_cox_runs_do_not_depend_on_rounding(run):
    r, rl = H.cox_reference(run), H.cox_reference(run, np.longdouble)
    assert _same(r, rl, ("flags", "iterations")), (r["flags"], rl["flags"], r["iterations"], rl["iterations"])
    _criteria_clear(r, 1e-9, run)
    for f, pv in enumerate(r["pivots"]):
        for d, limit in pv:
            assert abs(d - limit) > PIVOT_MARGIN * limit, (run, f, d, limit)
    out, fitted = _quarter(H.cox_tolerances(run)[0], r["flags"], run)
    print(f"{ids(run)}: {out} of {fitted} fits have est and se left out")


@pytest.mark.parametrize("run", H.SCORE_RUNS, ids=ids)
def test_score_runs_do_not_depend_on_rounding(run):
    Z, Zl = H.score_reference(run), H.score_reference(run, np.longdouble)
    assert Z.base["flags"] == Zl.base["flags"] and Z.base["iterations"] == Zl.base["iterations"]
    assert np.array_equal(Z.flags, Zl.flags) and np.array_equal(Z.df, Zl.df) and np.array_equal(Z.kept, Zl.kept)
    for c in Z.base["crit"]:
        assert abs(c - 1e-8) > CRIT_MARGIN * 1e-8
    for v in Z.ratios:
        assert not abs(v - 1e-11) <= PIVOT_MARGIN * 1e-11
    assert H.score_base_tolerance(run) <= H.LEFT_OUT_ABOVE       # the base fit's est and se are compared


def test_the_existing_cox_runs_keep_flags_and_iterations():
    """The pivots of tests/assocsurv_reference.py's own device runs: G_jj >= I_jj, so a pivot that passes against G_jj passed
    against I_jj; the rejected ones are exactly collinear or empty columns (no positive remainder), which failed before; and
    none is near the new threshold.  The closest are the monotone fits of the single-event case, whose information shrinks
    by e per iteration: 2.29 thresholds in iteration 20 (measured)."""
    smallest = np.inf
    for run in S.DEVICE_RUNS:
        r = S.reference(*run)
        for f, pv in enumerate(r["pivots"]):
            for d, limit in pv:
                if d > limit:
                    smallest = min(smallest, d / limit)
                else:
                    assert d <= 1e-3 * limit, (run, f, d, limit)
    assert smallest > 2, smallest
    print(f"the smallest accepted pivot of the existing runs: {smallest:.3g} thresholds")


def test_no_cox_fit_reports_a_runaway_coefficient():
    worst = 0.0
    for run in H.COX_RUNS:
        case, model, ties, cov, maxit = run
        c, r = H.cox_cohort(case), H.cox_reference(run)
        A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, model)
        slots = [(-1, -1)] + S.fit_slots(A.rsum, model, A.n)
        for f, rows in enumerate(slots):
            if rows is None or r["flags"][f] & S.RANK_BIT:
                continue
            eta = np.zeros(A.n)
            for i, row in enumerate(rows):
                if row >= 0:
                    eta = eta + r["coef"][f, i] * A.F[row]
            for j, col in enumerate(c["covar"][cov]):
                eta = eta + r["coef"][f, S.COV0 + j] * col
            worst = max(worst, float(np.abs(eta).max()))
            assert np.abs(eta).max() <= ETA_BOUND, (run, f, float(np.abs(eta).max()))
    assert 200 < worst <= ETA_BOUND < 1e88
    print(f"the largest |eta| of a reported Cox fit: {worst:.6g}")


# 4 where a finite maximum exists -----------------------------------------------------------------------------------------
def test_quasi_separated_rows_against_an_independent_mle():
    seen = 0
    for case in ("n40", "n255", "n257"):
        c = H.glm_cohort(case)
        run = (case, "dominant", "q0", False, 25, 1e-8)
        r = H.glm_reference(run)
        A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], "dominant")
        f = _row(c, "quasi")
        assert r["flags"][f] == 0
        b, se = glm_mle(np.stack([np.ones(A.n), A.F[f].astype(float)], axis=1), A.y.astype(float))
        for j, slot in enumerate((0, 1)):
            ge, gs = _gap(r["coef"][f, slot], r["se"][f, slot], b[j], se[j])
            assert ge <= EST_BOUND and gs <= SE_BOUND, (case, slot, ge, gs)
        seen += 1
    for run in H.COX_RUNS:
        case, model, ties, cov, maxit = run
        if model != "dominant" or maxit != 20 or cov not in ("q0", "q2"):
            continue
        c, r = H.cox_cohort(case), H.cox_reference(run)
        A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, model)
        for name in ("tie_block", "longest"):
            f = 1 + _row(c, name)
            if r["flags"][f] or r["iterations"][f] > 8:          # (the four longest follow-ups all censored: monotone)
                continue
            X = np.stack([A.F[f - 1].astype(float)] + list(c["covar"][cov]), axis=1)
            b, se = cox_mle(X, c["time"], A.y, ties)
            for j, slot in enumerate([0] + list(range(S.COV0, S.COV0 + len(c["covar"][cov])))):
                ge, gs = _gap(r["coef"][f, slot], r["se"][f, slot], b[j], se[j])
                assert ge <= EST_BOUND and gs <= SE_BOUND, (run, name, slot, ge, gs)
            seen += 1
    assert seen >= 10


# 5 end to end: the runs of the device tests on the restatement in both precisions ------------------------------------------
def test_end_to_end_runs_do_not_depend_on_rounding():
    class LongG(G.Backend):
        dtype = np.longdouble

    class LongS(S.Backend):
        dtype = np.longdouble

    hla, y, covar = H.glm_hla("n257")
    a = hb.hlaAssocGlm(hla, y, covar, use_prob=True, maxit=60, epsilon=1e-14, _backend=G.Backend)
    b = hb.hlaAssocGlm(hla, y, covar, use_prob=True, maxit=60, epsilon=1e-14, _backend=LongG)
    assert np.array_equal(a.flags, b.flags) and np.array_equal(a.iterations, b.iterations)
    assert set(a.flags.tolist()) >= {0, G.RANK_BIT, G.BOUNDARY_BIT}
    hla, time, event, covar = H.cox_hla("n257")
    a = hb.hlaAssocSurv(hla, time, event, covar, ties="breslow", _backend=S.Backend)
    b = hb.hlaAssocSurv(hla, time, event, covar, ties="breslow", _backend=LongS)
    assert np.array_equal(a.flags, b.flags) and np.array_equal(a.iterations, b.iterations)
    c = H.cox_cohort("n257")
    names = S.allele_names(c["n_allele"])
    for name in ("earliest_k", "earliest_1"):
        t = a.name.index(names[_row(c, name)])
        assert a.flags[t] == S.RANK_BIT and np.isnan(a.est[t, 0]) and np.isnan(a.lrt_p[t])
    assert all(abs(v - 1e-9) > 1e-15 for crits in S.Backend.last["crit"] for v in crits)


# 6 the tolerances hold the restatement to itself -------------------------------------------------------------------------
def _order_spread(kind, run):
    """(the largest difference in est / se between the float64 restatement and itself with the samples reordered, as a share
    of the fit's tolerance, over the fits whose est and se are compared; whether flags, iterations and dropped columns are
    the same in every order)."""
    import associnteract_reference as I
    case, model, cov, weighted, maxit, epsilon = run
    c = H.glm_cohort(case)
    A = AR.Analysis(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], model)
    ref = {"glm": H.glm_reference, "sets": H.sets_reference, "terms": H.terms_reference}[kind]
    want, wantl = ref(run), ref(run, np.longdouble)
    tol = H.wide_tolerances(want, wantl)[0]
    compared = ((want["flags"] & G.RANK_BIT) == 0) & (tol <= H.LEFT_OUT_ABOVE)
    share, same = 0.0, True
    for seed in (0, 1, 2):
        p = np.random.default_rng(seed).permutation(A.n)
        w = c["weight"][p] if weighted else None
        F, covar, y = A.F[:, p], c["covar"][cov][:, p], A.y[p]
        if kind == "glm":
            r = G.glm_rows(F, model, covar, w, y, maxit, epsilon)
        elif kind == "sets":
            r = O.glm_sets(F, H.glm_sets_of(case), covar, w, y, maxit, epsilon)
        else:
            r = I.glm_terms(F, H.glm_terms_of(case), covar, w, y, maxit, epsilon)
        same = same and _same(r, want, ("flags", "iterations") + (("df_h",) if kind != "glm" else ()))
        scale = np.fmax(np.abs(want["coef"]), want["se"])
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.fmax(np.nanmax(np.nan_to_num(np.abs(r["coef"] - want["coef"]) / scale), axis=1),
                        np.nanmax(np.nan_to_num(np.abs(r["se"] / want["se"] - 1)), axis=1))
        share = max(share, float((d / tol)[compared].max()))
    return share, same


@pytest.mark.parametrize("kind,run", [("glm", r) for r in H.GLM_RUNS] + [(k, r) for k in ("sets", "terms") for r in H.WIDE_RUNS],
                         ids=lambda v: v if isinstance(v, str) else ids(v))
def test_tolerances_hold_the_restatement_to_itself(kind, run):
    """The device sums in an order of its own, so a compared fit must not depend on the order of summation beyond its
    tolerance: the float64 restatement with the samples reordered (three orders) keeps flags, iterations and dropped columns,
    and moves est and se by at most a quarter of the fit's tolerance (the largest: 0.12).  Where two columns of a set are
    nearly collinear the one float64-versus-longdouble difference that the tolerance is taken from can be far smaller than
    the spread between orders; such a run is not part of the corpus."""
    share, same = _order_spread(kind, run)
    assert same and share <= 0.25, (kind, run, share, same)


@pytest.mark.parametrize("run", [r for r in H.COX_RUNS if r[0] != "n257u"], ids=ids)
def test_cox_tolerances_hold_the_restatement_to_itself(run):
    """The same for Cox, where only the order inside a tie block is free: the samples of every block reordered (three
    orders; the untied cohort has nothing to reorder).  Flags and iterations stay; est and se move by at most a quarter of
    the fit's tolerance."""
    case, model, ties, cov, maxit = run
    c, want = H.cox_cohort(case), H.cox_reference(run)
    A = AR.Analysis(c["a1"], c["a2"], c["event"], c["n_allele"], None, model)
    B = S.Blocks(c["time"])
    tol = H.cox_tolerances(run)[0]
    compared = ((want["flags"] & S.RANK_BIT) == 0) & (tol <= H.LEFT_OUT_ABOVE)
    share = 0.0
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        p = np.concatenate([rng.permutation(np.arange(B.first[k], B.first[k + 1])) for k in range(B.nb)])
        r = S.cox_rows(A.F[:, p], model, c["time"][p], c["covar"][cov][:, p], A.y[p], ties, maxit, 1e-9, start=c["start"].get(cov))
        assert _same(r, want, ("flags", "iterations")), (run, seed, r["flags"], want["flags"], r["iterations"], want["iterations"])
        scale = np.fmax(np.abs(want["coef"]), want["se"])
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.fmax(np.nanmax(np.nan_to_num(np.abs(r["coef"] - want["coef"]) / scale), axis=1),
                        np.nanmax(np.nan_to_num(np.abs(r["se"] / want["se"] - 1)), axis=1))
        share = max(share, float((d / tol)[compared].max()))
    assert share <= 0.25, (run, share)
