"""The hard cohorts of tests/assoc_hard_corpus.py on the GPU: separated and monotone-likelihood fits
through hibag_hip_assoc_glm, _glm_sets, _glm_terms, _assoc_cox and the score base fit against the restatements, and once end
to end through hlaAssocGlm and hlaAssocSurv.  Per fit, the fits with the rank bit included: flags, iterations, dropped columns
and the NaN pattern equal; deviance or log-likelihood, the score statistic, est and se within 100 x the restatement's
float64-versus-longdouble difference for that fit (at least 1e-12; so no wider than the run's); est and se, and only they,
left out of the value comparison where the fit's own tolerance exceeds 1e-6 -- a diverging fit's est and se are decided by its last bits --, at most a quarter of a run's
fits (tests/test_assoc_hard_host.py asserts the same count from the restatement alone); every call repeated, bit for bit.
The integer comparisons rest on the safety conditions that the host file asserts for every run here.

The last test prints, per kernel, the flag bits that a compared fit carried, the fits compared and left out and the largest
device difference as a share of its tolerance; DESIGN.md section 32 has the measured values."""
import numpy as np
import pytest

import hibag_amd as hb
import assoc_hard_corpus as H
import assoc_reference as AR
import assocglm_reference as G
import assocsurv_reference as S
from hibag_amd import _lib, assoc, assocglm, associnteract, assocomni, assocscore, assocsurv

pytestmark = pytest.mark.gpu

MODELS = AR.MODELS
ids = lambda run: "-".join(str(v) for v in run)                  # noqa: E731
SUMMARY = {}                                                     # kernel -> [flag bits seen, fits compared, est left out, worst share]


def bits_equal(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def compare(kernel, what, got, want, tol_est, tol_val, values, extra=()):
    """got, want: dicts with coef, se, iterations, flags, the ``values`` (deviance, or loglik and score) and the integer
    columns ``extra``; tol_est [n_fit] and tol_val {value: [n_fit]} per fit (no wider than the run's).  The iteration counts
    are compared for every fit: a fit that fails on a pivot reports the iteration it failed in, a fit that is not run 0."""
    assert np.array_equal(got["flags"], want["flags"]), (what, got["flags"], want["flags"])
    fitted = (want["flags"] & G.RANK_BIT) == 0
    assert np.array_equal(got["iterations"], want["iterations"]), (what, got["iterations"], want["iterations"])
    for k in extra:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("coef", "se") + tuple(values):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k)
    assert np.isnan(got["coef"][~fitted]).all() and np.isnan(got["se"][~fitted]).all(), what
    out, n_fitted = H.left_out(tol_est, want["flags"])
    assert 4 * int(out.sum()) <= n_fitted, (what, int(out.sum()), n_fitted)
    share = 0.0
    scale = np.fmax(np.abs(want["coef"]), want["se"])
    with np.errstate(invalid="ignore", divide="ignore"):
        d_est = np.nanmax(np.nan_to_num(np.abs(got["coef"] - want["coef"]) / scale), axis=1)
        d_se = np.nanmax(np.nan_to_num(np.abs(got["se"] / want["se"] - 1)), axis=1)
        d_val = {k: np.nan_to_num(np.abs(got[k] / want[k] - 1)) for k in values}
    cmp_est = fitted & ~out
    line = [f"{what}: {n_fitted} fits, est and se of {int(out.sum())} left out"]
    if cmp_est.any():
        s_est = float(np.max(np.fmax(d_est, d_se)[cmp_est] / tol_est[cmp_est]))
        share = max(share, s_est)
        line.append(f"est {d_est[cmp_est].max():.3g} se {d_se[cmp_est].max():.3g} ({s_est:.3g} of tol)")
    for k in values:
        dv = float(d_val[k][fitted].max()) if fitted.any() else 0.0
        share = max(share, float((d_val[k] / tol_val[k])[fitted].max()) if fitted.any() else 0.0)
        line.append(f"{k} {dv:.3g} (tol {tol_val[k][fitted].min():.3g} ... {tol_val[k][fitted].max():.3g})")
    print(", ".join(line) + f", at most {int(got['iterations'].max())} iterations")
    rec = SUMMARY.setdefault(kernel, [0, 0, 0, 0.0])
    rec[0] |= int(np.bitwise_or.reduce(want["flags"]))
    rec[1], rec[2], rec[3] = rec[1] + n_fitted, rec[2] + int(out.sum()), max(rec[3], share)
    assert (np.fmax(d_est, d_se)[cmp_est] <= tol_est[cmp_est]).all(), (what, d_est, d_se, tol_est)
    for k in values:
        assert (d_val[k][fitted] <= tol_val[k][fitted]).all(), (what, k, d_val[k], tol_val[k])


# 1 the narrow kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", H.GLM_RUNS, ids=ids)
def test_glm_fits_equal_the_restatement(run):
    case, model, cov, weighted, maxit, epsilon = run
    c, want = H.glm_cohort(case), H.glm_reference(run)
    tol_est, tol_dev = H.glm_tolerances(run)
    with assocglm._DeviceGlm(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], MODELS.index(model)) as dev:
        assert dev.n_kept == len(c["y"])
        first = dev.glm(c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon)
        assert bits_equal(first, dev.glm(c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon))
    got = dict(zip(("coef", "se", "deviance", "iterations", "flags"), first))
    compare("k_glm_fit", "glm " + ids(run), got, want, tol_est, {"deviance": tol_dev}, ("deviance",))


# 2 the wide and the terms kernel -----------------------------------------------------------------------------------------
WIDE_OUT = ("coef", "se", "deviance", "iterations", "flags", "df_h")


@pytest.mark.parametrize("run", H.WIDE_RUNS, ids=ids)
def test_set_fits_equal_the_restatement(run):
    case, model, cov, weighted, maxit, epsilon = run
    c, want, wantl = H.glm_cohort(case), H.sets_reference(run), H.sets_reference(run, np.longdouble)
    tol_est, tol_dev = H.wide_tolerances(want, wantl)
    with assocomni._DeviceOmni(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], MODELS.index(model)) as dev:
        first = dev.glm_sets(H.glm_sets_of(case), c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon)
        assert bits_equal(first, dev.glm_sets(H.glm_sets_of(case), c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon))
    compare("k_glm_fit wide", "sets " + ids(run), dict(zip(WIDE_OUT, first)), want, tol_est, {"deviance": tol_dev}, ("deviance",), extra=("df_h",))


@pytest.mark.parametrize("run", H.WIDE_RUNS, ids=ids)
def test_term_fits_equal_the_restatement(run):
    case, model, cov, weighted, maxit, epsilon = run
    c, want, wantl = H.glm_cohort(case), H.terms_reference(run), H.terms_reference(run, np.longdouble)
    tol_est, tol_dev = H.wide_tolerances(want, wantl)
    with associnteract._DeviceInteract(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], MODELS.index(model)) as dev:
        first = dev.glm_terms(H.glm_terms_of(case), c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon)
        assert bits_equal(first, dev.glm_terms(H.glm_terms_of(case), c["covar"][cov], c["weight"] if weighted else None, maxit, epsilon))
    compare("terms kernel", "terms " + ids(run), dict(zip(WIDE_OUT, first)), want, tol_est, {"deviance": tol_dev}, ("deviance",), extra=("df_h",))


# 3 Cox ---------------------------------------------------------------------------------------------------------------------
def device_cox(dev, c, ties, cov, maxit):
    start = c["start"].get(cov)
    if start is None:
        return dev.cox(c["time"], c["covar"][cov], S.TIES.index(ties), maxit, 1e-9)
    p, n_fit = assoc._ptr, dev.n_tests + 1
    covar = np.ascontiguousarray(c["covar"][cov], np.float64)
    coef, se = np.empty((n_fit, 16)), np.empty((n_fit, 16))
    ll, sc, it, fl = np.empty(n_fit), np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
    _lib.check(_lib.lib().hibag_hip_assoc_cox(dev._h, p(np.ascontiguousarray(c["time"])), p(covar), len(covar), S.TIES.index(ties), maxit, 1e-9,
                                              p(np.ascontiguousarray(start, np.float64)), p(coef), p(se), p(ll), p(sc), p(it), p(fl)))
    return coef, se, ll, sc, it, fl


@pytest.mark.parametrize("run", H.COX_RUNS, ids=ids)
def test_cox_fits_equal_the_restatement(run):
    case, model, ties, cov, maxit = run
    c, want = H.cox_cohort(case), H.cox_reference(run)
    tol_est, tol_ll, tol_sc = H.cox_tolerances(run)
    with assocsurv._DeviceSurv(c["a1"], c["a2"], c["event"], c["n_allele"], None, MODELS.index(model)) as dev:
        assert dev.n_kept == len(c["time"])
        first = device_cox(dev, c, ties, cov, maxit)
        assert bits_equal(first, device_cox(dev, c, ties, cov, maxit))
    got = dict(zip(("coef", "se", "loglik", "score", "iterations", "flags"), first))
    compare("k_cox_fit", "cox " + ids(run), got, want, tol_est, {"loglik": tol_ll, "score": tol_sc}, ("loglik", "score"))


def test_a_collapsed_information_has_the_rank_bit():
    """The carriers are the earliest events: judged against G_jj the pivot of I = G - V fails on the device as in the
    restatement, in the same iteration; no such fit reports a coefficient."""
    c = H.cox_cohort("n257")
    want = H.cox_reference(("n257", "dominant", "efron", "q0", 20))
    with assocsurv._DeviceSurv(c["a1"], c["a2"], c["event"], c["n_allele"], None, 0) as dev:
        coef, se, ll, sc, it, fl = dev.cox(c["time"], None, 0, 20, 1e-9)
    for name in ("earliest_k", "earliest_1"):
        f = 1 + H.row(c, name)
        assert fl[f] == S.RANK_BIT and it[f] == want["iterations"][f] >= 2 and np.isnan(coef[f]).all() and np.isnan(ll[f]), (name, fl[f], it[f])
    assert np.nanmax(np.abs(coef)) < 100


# 4 the score base fit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", H.SCORE_RUNS, ids=ids)
def test_score_base_fit_equals_the_restatement(run):
    case, cov, weighted, maxit = run
    c, Z, Zl = H.glm_cohort(case), H.score_reference(run), H.score_reference(run, np.longdouble)
    tol = H.score_base_tolerance(run)
    q = len(c["covar"][cov])
    used = [0] + list(range(G.COV0, G.COV0 + q))
    with assocscore._DeviceScore(c["a1"], c["a2"], c["y"], c["n_allele"], c["g"], 0) as dev:
        dev.score(c["covar"][cov], c["weight"] if weighted else None, maxit, 1e-8)
        first = dev.score_base()
        assert bits_equal(first[:2], dev.score_base()[:2]) and first[2:] == dev.score_base()[2:]
        coef, se, deviance, it, fl = first
        proj, Smat, kept = dev.score_sets(H.score_sets_of(case))
        g, stat, df, flags = dev.score_observed()
    assert fl == Z.base["flags"] and it == Z.base["iterations"]
    assert np.isfinite(coef[used]).all() and np.isnan(np.delete(coef, used)).all() and np.isnan(np.delete(se, used)).all()
    b = {k: np.asarray(Z.base[k], np.float64) for k in ("coef", "se")}
    d_est = np.max(np.abs(coef[used] - b["coef"]) / np.fmax(np.abs(b["coef"]), b["se"]))
    d_se, d_dev = np.max(np.abs(se[used] / b["se"] - 1)), abs(deviance / float(Z.base["deviance"]) - 1)
    want_stat = np.asarray(Z.stat, np.float64)
    with np.errstate(invalid="ignore"):
        tol_stat = max(100.0 * float(np.nanmax(np.nan_to_num(np.abs(want_stat / np.asarray(Zl.stat, np.float64) - 1)))), 1e-12)
        d_stat = float(np.nanmax(np.nan_to_num(np.abs(stat / want_stat - 1))))
    print(f"score {ids(run)}: base flags {fl} after {it} iterations, tol {tol:.3g}, device differences est {d_est:.3g} se {d_se:.3g} "
          f"deviance {d_dev:.3g} ({max(d_est, d_se, d_dev) / tol:.3g} of tol); statistics {d_stat:.3g} (tol {tol_stat:.3g})")
    rec = SUMMARY.setdefault("score base fit", [0, 0, 0, 0.0])
    rec[0], rec[1], rec[3] = rec[0] | fl, rec[1] + 1, max(rec[3], max(d_est, d_se, d_dev) / tol)
    assert max(d_est, d_se, d_dev) <= tol
    assert np.array_equal(flags, Z.flags) and np.array_equal(df, Z.df) and np.array_equal(kept, Z.kept), (flags, Z.flags, df, Z.df)
    assert np.array_equal(np.isnan(stat), np.isnan(want_stat)) and d_stat <= tol_stat
    if cov == "sep":                                             # the failure path: bit 0 on every test, no statistic
        assert fl & G.MAXIT_BIT and (flags & 1).all() and (df == 0).all() and np.isnan(stat).all()


# 5 end to end ----------------------------------------------------------------------------------------------------------------
def _columns(res, keys):
    return {k: np.asarray(getattr(res, k), np.float64) for k in keys}


def _end_to_end(what, got, want, long, value):
    """Names, flags, iterations (of every test) and the NaN pattern of every column equal; the value column and est and se
    within each fit's own tolerance, as in ``compare``."""
    assert got.name == want.name and np.array_equal(got.flags, want.flags), (what, got.flags, want.flags)
    fitted = (want.flags & 2) == 0
    assert np.array_equal(got.iterations, want.iterations), (what, got.iterations, want.iterations)
    keys = ("est", "se", "lower", "upper", "pval", value, "lrt_stat", "lrt_p")
    g, w, wl = _columns(got, keys), _columns(want, keys), _columns(long, keys)
    for k in keys:
        assert np.array_equal(np.isnan(g[k]), np.isnan(w[k])), (what, k)
    assert np.isnan(g["est"][~fitted]).all() and np.isnan(g["lrt_p"][~fitted]).all()
    scale = np.fmax(np.abs(wl["est"]), wl["se"])
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_est = np.fmax(100.0 * np.nanmax(np.nan_to_num(np.fmax(np.abs(w["est"] - wl["est"]) / scale, np.abs(w["se"] / wl["se"] - 1))), axis=1), 1e-12)
        tol_val = np.fmax(100.0 * np.nan_to_num(np.abs(w[value] / wl[value] - 1)), 1e-12)
        d = np.nanmax(np.nan_to_num(np.fmax(np.abs(g["est"] - w["est"]) / np.fmax(np.abs(w["est"]), w["se"]), np.abs(g["se"] / w["se"] - 1))), axis=1)
        d_val = np.nan_to_num(np.abs(g[value] / w[value] - 1))
    out, n_fitted = H.left_out(tol_est, want.flags)
    assert 4 * int(out.sum()) <= n_fitted
    cmp_est = fitted & ~out
    print(f"{what}: {n_fitted} fits, est and se of {int(out.sum())} left out, est / se {float((d / tol_est)[cmp_est].max()):.3g} of tol, "
          f"{value} {float(d_val.max()):.3g} (tol {float(tol_val[fitted].min()):.3g} ... {float(tol_val[fitted].max()):.3g})")
    assert (d[cmp_est] <= tol_est[cmp_est]).all() and (d_val <= tol_val).all()
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]


def test_hla_assoc_glm_end_to_end():
    class Long(G.Backend):
        dtype = np.longdouble

    hla, y, covar = H.glm_hla("n257")
    kw = dict(use_prob=True, maxit=60, epsilon=1e-14)
    want = hb.hlaAssocGlm(hla, y, covar, _backend=G.Backend, **kw)
    got = hb.hlaAssocGlm(hla, y, covar, **kw)
    _end_to_end("hlaAssocGlm n257 weighted, 60 iterations", got, want, hb.hlaAssocGlm(hla, y, covar, _backend=Long, **kw), "deviance")
    c = H.glm_cohort("n257")
    names = G.allele_names(c["n_allele"])
    by = {v: got.name.index(names[k]) for k, v in c["names"].items()}
    assert got.flags[by["zero_weight"]] == G.RANK_BIT and np.isnan(got.pval[by["zero_weight"], 0])
    assert got.flags[by["all_cases"]] == G.BOUNDARY_BIT and got.est[by["all_cases"], 0] > 25 and got.se[by["all_cases"], 0] > 1e3
    assert got.flags[by["all_controls"]] == G.BOUNDARY_BIT and got.est[by["all_controls"], 0] < -25
    assert got.flags[by["quasi"]] == 0 and got.flags[by["tiny_weight"]] == 0


def test_hla_assoc_surv_end_to_end():
    class Long(S.Backend):
        dtype = np.longdouble

    hla, time, event, covar = H.cox_hla("n257")
    want = hb.hlaAssocSurv(hla, time, event, covar, ties="breslow", _backend=S.Backend)
    got = hb.hlaAssocSurv(hla, time, event, covar, ties="breslow")
    _end_to_end("hlaAssocSurv n257 breslow", got, want, hb.hlaAssocSurv(hla, time, event, covar, ties="breslow", _backend=Long), "loglik")
    c = H.cox_cohort("n257")
    names = S.allele_names(c["n_allele"])
    by = {v: got.name.index(names[k]) for k, v in c["names"].items()}
    for name in ("earliest_k", "earliest_1"):
        t = by[name]
        assert got.flags[t] == S.RANK_BIT and np.isnan(got.est[t, 0]) and np.isnan(got.lrt_p[t]) and np.isnan(got.score_p[t])
        assert got.carrier_events[t, 0] == got.carriers[t, 0] > 0
    assert got.flags[by["all_censored"]] == 0 and got.est[by["all_censored"], 0] < -10 and got.carrier_events[by["all_censored"], 0] == 0
    assert got.flags[by["tie_block"]] == 0


# 6 the summary ---------------------------------------------------------------------------------------------------------------
def test_summary():
    """Per kernel what the runs above compared.  Where all of them ran in this process: every flag bit the kernel can set was
    carried by a compared fit, and the left-out share is under a quarter."""
    for kernel, (flags, fits, out, share) in SUMMARY.items():
        print(f"{kernel}: flag bits {flags:#x} compared, {fits} fits, est and se of {out} left out ({out / max(fits, 1):.1%}), "
              f"largest device difference {share:.3g} of its tolerance")
        assert 4 * out <= fits
    want = {"k_glm_fit": 7, "k_glm_fit wide": 15, "terms kernel": 15, "k_cox_fit": 15, "score base fit": 5}
    if all(k in SUMMARY for k in want):
        for kernel, bits in want.items():
            assert SUMMARY[kernel][0] & bits == bits, (kernel, SUMMARY[kernel][0], bits)
