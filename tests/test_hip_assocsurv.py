"""hlaAssocSurv on the GPU: hibag_hip_assoc_cox against the restatement (tests/assocsurv_reference.py: DESIGN.md section 31
in numpy) -- iterations and flags equal, estimates, standard errors, log-likelihoods and score statistics within a tolerance
computed from the restatement alone (100 x its float64-versus-longdouble difference over the case's fits, at least 1e-12) --:
the six-subject example, cohorts around a 256-sample boundary with ten distinct times, cohorts that end one matrix-core step
below and above a seam between two waves' segments with a tie block across every seam, a block of more than 64 events, all
samples at one time, the longest follow-ups all censored, a single event; both ties rules, the four models, maxit = 2;
hlaAssocSurv end to end, conditioned on its top hit; results bit-equal across calls and handles; invalid arguments rejected.

Measured (DESIGN.md section 31 has the table per case): the largest device difference is 3.8 % of its case's tolerance (n257,
score 2.0e-13 relative against 5.3e-12); where the tolerance is the floor of 1e-12 the device is within 4e-14."""
import ctypes as C

import numpy as np
import pytest

import hibag_amd as hb
import assoc_reference as AR
import assocsurv_reference as S
from hibag_amd import _lib, assoc, assocsurv

pytestmark = pytest.mark.gpu

MODELS, TIES = S.MODELS, S.TIES


def device_cox(case, model, ties="efron", maxit=20, alleles_only=False):
    c = S.device_cohort(case)
    with assocsurv._DeviceSurv(c["a1"], c["a2"], c["event"], c["n_allele"], None if alleles_only else c["g"], MODELS.index(model)) as dev:
        assert dev.n_kept == len(c["time"])
        return dev.cox(c["time"], c["covar"], TIES.index(ties), maxit, 1e-9)


def compare(got, want, tol, what):
    """The value comparison of section 31: flags and iterations equal; fits without the rank bit within tol; the others NaN."""
    coef, se, ll, sc, it, fl = got
    assert np.array_equal(fl, want["flags"]), (what, fl, want["flags"])
    fitted = (want["flags"] & S.RANK_BIT) == 0
    assert np.array_equal(it[fitted], want["iterations"][fitted]), (what, it, want["iterations"])
    assert np.array_equal(np.isnan(coef), np.isnan(want["coef"])) and np.array_equal(np.isnan(se), np.isnan(want["se"])), what
    assert np.array_equal(np.isnan(sc), np.isnan(want["score"])) and np.array_equal(np.isnan(ll), np.isnan(want["loglik"])), what
    assert np.isnan(ll[~fitted]).all() and np.isnan(coef[~fitted]).all() and np.isnan(se[~fitted]).all() and np.isnan(sc[~fitted]).all(), what
    d_est, d_se, d_ll, d_sc = S.gaps(dict(coef=coef, se=se, loglik=ll, score=sc), want)
    print(f"{what}: tol {tol:.3g}, device differences est {d_est:.3g} se {d_se:.3g} loglik {d_ll:.3g} score {d_sc:.3g} "
          f"({max(d_est, d_se, d_ll, d_sc) / tol:.3g} of tol), {int(fitted.sum())} fits, at most {int(it.max())} iterations")
    assert d_est <= tol and d_se <= tol and d_ll <= tol and d_sc <= tol, what


# 1 values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(S.CASES))
def test_fits_equal_the_restatement(case, model, ties):
    want = S.reference(case, model, ties)
    compare(device_cox(case, model, ties), want, S.tolerance(case, model, ties), f"{case} {model} {ties}")


def test_the_cases_are_what_they_claim():
    step, seg = S.segment_of(400)
    assert step == 4 and seg % step == 0
    for case, last in (("seam_lo", S.SEAM * seg - step), ("seam_hi", S.SEAM * seg + step)):
        c = S.device_cohort(case)
        B = S.Blocks(c["time"])
        assert len(c["time"]) == last and S.segment_of(last) == (step, seg)
        for w in range(1, S.SEAM + (case == "seam_hi")):         # a block with events on both sides lies across every seam
            k = B.blk[w * seg]
            assert B.blk[w * seg - 1] == k and B.first[k] <= w * seg - 3 and B.first[k + 1] >= w * seg + 3
    c = S.device_cohort("n1000")
    B = S.Blocks(c["time"])
    kept, = AR.kept_columns(c["a1"], c["a2"], c["event"])
    assert np.add.reduceat(kept, B.first[:-1]).max() > 64 and S.segment_of(len(kept))[1] == 128
    assert np.diff(B.first).max() < 128                          # (inside a segment or across one seam)
    c = S.device_cohort("one_time")                              # one block, larger than a segment, across every seam
    assert S.Blocks(c["time"]).nb == 1 and len(c["time"]) > S.segment_of(len(c["time"]))[1]
    c = S.device_cohort("late_censored")
    kept, = AR.kept_columns(c["a1"], c["a2"], c["event"])
    assert kept[:15].sum() == 0 and kept.sum() > 10
    c = S.device_cohort("one_event")
    assert AR.kept_columns(c["a1"], c["a2"], c["event"])[0].sum() == 1
    for case in ("n255", "n256", "n257"):
        assert S.Blocks(S.device_cohort(case)["time"]).nb <= 10
    assert S.Blocks(S.device_cohort("n40")["time"]).nb == 37
    assert (S.device_cohort("n1000")["a1"] == AR.NA_INTEGER).sum() + (S.device_cohort("n1000")["a2"] == AR.NA_INTEGER).sum() == 3


def test_the_six_subject_example():
    """Breslow: beta = log((3 + sqrt 33) / 2); allele 1 is carried by everybody: rank bit."""
    coef, se, ll, sc, it, fl = device_cox("n6", "dominant", "breslow")
    assert abs(coef[1, 0] - np.log((3 + np.sqrt(33)) / 2)) <= 1e-9 and fl.tolist() == [0, 0, 2] and np.isnan(coef[2]).all()
    assert abs(sc[1] - 1.6) <= 1e-12 and it[0] == 0 and np.isnan(coef[0]).all()


@pytest.mark.parametrize("model", MODELS)
def test_maxit_2(model):
    want = S.reference("n257", model, maxit=2)
    assert (want["flags"] & S.MAXIT_BIT).any()
    compare(device_cox("n257", model, maxit=2), want, S.tolerance("n257", model, maxit=2), f"n257 {model} maxit 2")


def test_rank_deficient_and_no_event_fits():
    want = S.reference("n1000", "genotype")
    assert (want["flags"] & S.RANK_BIT).sum() >= 1                # the partition's empty level
    c = S.device_cohort("n257")
    cov = np.concatenate([c["covar"][:3], c["covar"][:1] * 2.0])  # collinear covariates: the base model fails, and all with it
    with assocsurv._DeviceSurv(c["a1"], c["a2"], c["event"], c["n_allele"], None, 0) as dev:
        coef, se, ll, sc, it, fl = dev.cox(c["time"], cov, 0, 20, 1e-9)
        assert (fl == 2).all() and np.isnan(coef).all() and np.isnan(se).all() and np.isnan(ll).all() and np.isnan(sc).all()
    with assocsurv._DeviceSurv(c["a1"], c["a2"], np.zeros_like(c["event"]), c["n_allele"], None, 0) as dev:
        coef, se, ll, sc, it, fl = dev.cox(c["time"], c["covar"], 0, 20, 1e-9)
        assert (fl == 2).all() and (it == 0).all() and np.isnan(coef).all() and np.isnan(ll).all()


# 2 end to end ----------------------------------------------------------------------------------------------------
def assert_results_close(got, want, tol):
    assert got.name == want.name and np.array_equal(got.flags, want.flags)
    assert (got.n_samp, got.n_event, got.n_excluded) == (want.n_samp, want.n_event, want.n_excluded)
    for key in ("n", "events", "carriers", "carrier_events"):
        assert np.array_equal(getattr(got, key), getattr(want, key)), key
    ok = (want.flags & 2) == 0
    assert ok.sum() >= 10 and np.array_equal(got.iterations[ok], want.iterations[ok])
    for key in ("est", "se", "lower", "upper", "pval", "loglik", "lrt_stat", "lrt_p", "score_stat", "score_p"):
        assert np.array_equal(np.isnan(getattr(got, key)), np.isnan(getattr(want, key))), key
    scale = np.fmax(np.abs(want.est), want.se)
    assert np.nanmax(np.abs(got.est - want.est) / scale) <= tol and np.nanmax(np.abs(got.se / want.se - 1)) <= tol
    assert np.nanmax(np.abs(got.loglik / want.loglik - 1)) <= tol and np.nanmax(np.abs(got.score_stat / want.score_stat - 1)) <= tol
    # what follows on the host: the bounds from est and se; z = est / se moves by 2 tol (1 + |z|), the p-values with it
    assert np.nanmax(np.abs(got.lower - want.lower) / scale) <= 3 * tol and np.nanmax(np.abs(got.upper - want.upper) / scale) <= 3 * tol
    z = np.abs(want.est / want.se)
    fin = np.isfinite(z)
    assert (np.abs(np.log(got.pval[fin] / want.pval[fin])) <= 4 * tol * (1 + z[fin]) ** 2 + 1e-12).all()
    ll_scale = 2 * tol * (np.abs(want.loglik) + abs(want.base["loglik"]))
    fin = np.isfinite(want.lrt_stat)
    assert (np.abs(got.lrt_stat - want.lrt_stat)[fin] <= ll_scale[fin]).all()
    big = fin & (want.lrt_stat > 1e-3)                          # (the tail's log-derivative in the statistic is at most ~ 1 / stat + 1 / 2)
    assert (np.abs(np.log(got.lrt_p[big] / want.lrt_p[big])) <= ll_scale[big] * (1 / want.lrt_stat[big] + 1) + 1e-12).all()
    big = np.isfinite(want.score_p) & (want.score_stat > 1e-3)
    assert (np.abs(np.log(got.score_p[big] / want.score_p[big])) <= tol * want.score_stat[big] * (1 / want.score_stat[big] + 1) + 1e-12).all()
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]
    b = np.fmax(np.abs(want.base["est"]), want.base["se"])
    assert (np.abs(got.base["est"] - want.base["est"]) <= tol * b).all() and (np.abs(got.base["se"] / want.base["se"] - 1) <= tol).all()
    assert abs(got.base["loglik"] / want.base["loglik"] - 1) <= tol


def test_hla_assoc_surv_end_to_end_and_conditioned():
    hla, time, event, groups, covar = S.hla_of("n1000")
    tol = S.tolerance("n1000", "dominant")
    want = hb.hlaAssocSurv(hla, time, event, covar, groups=groups, _backend=S.Backend)
    got = hb.hlaAssocSurv(hla, time, event, covar, groups=groups)
    assert_results_close(got, want, tol)
    assert got.flags[-1] == 2 and got.name[-1] == "pos:beyond"                  # a level the device does not know
    top = got.name[int(np.nanargmin(got.pval[:, 0]))]
    assert top == want.name[int(np.nanargmin(want.pval[:, 0]))]
    cwant = hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=[top], show_hr=True, _backend=S.Backend)
    ctol = max(100.0 * max(S.gaps(S.Backend.last, _longdouble_of(hla, time, event, covar, groups, top))), 1e-12)
    cgot = hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=[top], show_hr=True)
    assert cgot.flags[got.name.index(top)] & 2 and cgot.base["name"][-1] == f"h[{top}]"
    for r in (cgot, cwant):                                                    # (hazard ratios: compared as logs)
        r.est, r.lower, r.upper = np.log(r.est), np.log(r.lower), np.log(r.upper)
    assert_results_close(cgot, cwant, ctol)
    # the genotype model under Breslow's rule
    hla, time, event, groups, covar = S.hla_of("n257")
    assert_results_close(hb.hlaAssocSurv(hla, time, event, covar, model="genotype", ties="breslow"),
                         hb.hlaAssocSurv(hla, time, event, covar, model="genotype", ties="breslow", _backend=S.Backend),
                         S.tolerance("n257", "genotype", "breslow"))


def _longdouble_of(hla, time, event, covar, groups, top):
    """The conditioned run on the restatement in longdouble (for its tolerance)."""
    class Long(S.Backend):
        dtype = np.longdouble
    hb.hlaAssocSurv(hla, time, event, covar, groups=groups, condition=[top], _backend=Long)
    return Long.last


# 3 reproducibility -----------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["dominant", "genotype"])
def test_results_are_bit_equal(model):
    """The same call twice; a handle with the alleles alone against one with the partition's tests beside them."""
    first = device_cox("n1000", model)
    assert bits_equal(first, device_cox("n1000", model))
    n_allele = S.CASES["n1000"][1]
    alone = device_cox("n1000", model, alleles_only=True)
    assert len(alone[2]) == n_allele + 1 and len(first[2]) > n_allele + 1
    assert bits_equal(alone, [a[:n_allele + 1] for a in first])


# 4 errors --------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0], np.int32)
    b = np.array([0, 0, 1, 1, 0, 1], np.int32)
    y = np.array([0, 1, 0, 1, 1, 0], np.int32)
    t = np.array([9.0, 8.0, 8.0, 5.0, 2.0, 0.0])
    with assocsurv._DeviceSurv(a, b, y, 2, None, 0) as dev:
        n_fit = dev.n_tests + 1
        coef, se = np.empty((n_fit, 16)), np.empty((n_fit, 16))
        ll, sc, it, fl = np.empty(n_fit), np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        cov = np.arange(13 * 6, dtype=np.float64).reshape(13, 6) % 5
        cov -= cov.mean(axis=1, keepdims=True)
        outs = (p(coef), p(se), p(ll), p(sc), p(it), p(fl))
        cox = L.hibag_hip_assoc_cox
        assert cox(dev._h, p(t), p(cov), 1, 0, 20, 1e-9, None, *outs) == 0 and np.isfinite(ll[0])
        assert cox(dev._h, p(t), None, 0, 1, 20, 1e-9, None, *outs) == 0 and it[0] == 0
        assert cox(dev._h, p(t), p(cov), 1, 0, 20, 1e-9, p(np.array([0.1])), *outs) == 0
        assert cox(dev._h, p(t), p(cov), 13, 0, 20, 1e-9, None, *outs) == -1 and b"13 covariates" in L.hibag_hip_last_error()
        assert cox(dev._h, p(t), p(cov), -1, 0, 20, 1e-9, None, *outs) == -1
        assert cox(dev._h, p(t), None, 1, 0, 20, 1e-9, None, *outs) == -1
        unsorted = t.copy()
        unsorted[3] = 8.5
        assert cox(dev._h, p(unsorted), p(cov), 1, 0, 20, 1e-9, None, *outs) == -1 and b"time order" in L.hibag_hip_last_error()
        for v in (-1.0, np.nan, np.inf):
            bad = t.copy()
            bad[0 if v != -1.0 else 5] = v
            assert cox(dev._h, p(bad), p(cov), 1, 0, 20, 1e-9, None, *outs) == -1 and b"finite and >= 0" in L.hibag_hip_last_error()
        for ties in (-1, 2):
            assert cox(dev._h, p(t), p(cov), 1, ties, 20, 1e-9, None, *outs) == -1 and b"ties" in L.hibag_hip_last_error()
        assert cox(dev._h, p(t), p(cov), 1, 0, 0, 1e-9, None, *outs) == -1 and b"maxit" in L.hibag_hip_last_error()
        for eps in (0.0, -1.0, float("nan")):
            assert cox(dev._h, p(t), p(cov), 1, 0, 20, eps, None, *outs) == -1 and b"epsilon" in L.hibag_hip_last_error()
        bad = cov.copy()
        bad[1, 2] = np.nan
        assert cox(dev._h, p(t), p(bad), 2, 0, 20, 1e-9, None, *outs) == -1 and b"not finite" in L.hibag_hip_last_error()
        assert cox(dev._h, p(t), p(cov), 1, 0, 20, 1e-9, p(np.array([np.nan])), *outs) == -1 and b"start" in L.hibag_hip_last_error()
        for k in range(6):
            o = list(outs)
            o[k] = None
            assert cox(dev._h, p(t), p(cov), 1, 0, 20, 1e-9, None, *o) == -1
        assert cox(dev._h, None, p(cov), 1, 0, 20, 1e-9, None, *outs) == -1
        assert cox(None, p(t), p(cov), 1, 0, 20, 1e-9, None, *outs) == -1 and b"hibag_hip_assoc_cox" in L.hibag_hip_last_error()
    step, seg = C.c_int(), C.c_int()
    assert L.hibag_hip_assoc_cox_segment(0, C.byref(step), C.byref(seg)) == -1
    assert L.hibag_hip_assoc_cox_segment(1000, C.byref(step), C.byref(seg)) == 0 and (step.value, seg.value) == (4, 128)
