"""hlaAssocGlm on the GPU: hibag_hip_assoc_glm against the restatement (tests/assocglm_reference.py: DESIGN.md section 23 in
numpy) -- iterations and flags equal, estimates, standard errors and deviances within a tolerance computed from the
restatement alone (100 x its float64-versus-longdouble difference over the case's fits, at least 1e-12) --, at cohort
sizes around a 256-sample boundary, for the four models, with maxit = 2, prior weights with zeros and an empty genotype
class; the feature rows byte for byte; hlaAssocGlm end to end, conditioned on its top hit; results bit-equal across calls,
handles and a permutation call in between; invalid arguments rejected.

Measured: the largest device difference is 2.2 % of its case's tolerance (n256 genotype, se 3.4e-11
relative against 1.5e-9); where the tolerance is the floor of 1e-12 the device is within 5.6e-15."""
import numpy as np
import pytest

import hibag_amd as hb
import assoc_reference as AR
import assocglm_reference as G
from hibag_amd import _lib, assoc, assocglm

pytestmark = pytest.mark.gpu

MODELS = G.MODELS


def device_glm(case, model, weighted=False, maxit=25, alleles_only=False, permute_first=False):
    n, n_allele, q, seed, part = G.CASES[case]
    a1, a2, y, g, covar, prob = G.cohort(n, n_allele, q, seed, part)
    covar, prob = G.kept_columns(a1, a2, covar, prob)
    with assocglm._DeviceGlm(a1, a2, y, n_allele, None if alleles_only else g, MODELS.index(model)) as dev:
        assert dev.n_kept == n - 3 == _lib.lib().hibag_hip_assoc_n_kept(dev._h)
        if permute_first:
            before = dev.glm(covar, prob if weighted else None, maxit, 1e-8)
            dev.permute(11, 1, 300)
            return before, dev.glm(covar, prob if weighted else None, maxit, 1e-8)
        return dev.glm(covar, prob if weighted else None, maxit, 1e-8)


def compare(got, want, tol, what):
    """The value comparison of section 23: flags and iterations equal; fits without the rank bit within tol; the others NaN."""
    coef, se, dev, it, fl = got
    assert np.array_equal(fl, want["flags"]), (what, fl, want["flags"])
    fitted = (want["flags"] & G.RANK_BIT) == 0
    assert np.array_equal(it[fitted], want["iterations"][fitted]), (what, it, want["iterations"])
    assert np.array_equal(np.isnan(coef), np.isnan(want["coef"])) and np.array_equal(np.isnan(se), np.isnan(want["se"])), what
    assert np.isnan(dev[~fitted]).all() and np.isnan(coef[~fitted]).all() and np.isnan(se[~fitted]).all(), what
    scale = np.fmax(np.abs(want["coef"]), want["se"])
    with np.errstate(invalid="ignore"):
        d_est = np.nanmax((np.abs(coef - want["coef"]) / scale)[fitted])
        d_se = np.nanmax(np.abs(se / want["se"] - 1)[fitted])
        d_dev = np.nanmax(np.abs(dev / want["deviance"] - 1)[fitted])
    print(f"{what}: tol {tol:.3g}, device differences est {d_est:.3g} se {d_se:.3g} deviance {d_dev:.3g} "
          f"({max(d_est, d_se, d_dev) / tol:.3g} of tol), {int(fitted.sum())} fits, at most {int(it.max())} iterations")
    assert d_est <= tol and d_se <= tol and d_dev <= tol, what


# 1 values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(G.CASES))
def test_fits_equal_the_restatement(case, model):
    want = G.reference(case, model)
    assert ((want["flags"] & G.RANK_BIT) == 0).sum() >= 4
    compare(device_glm(case, model), want, G.tolerance(case, model), f"{case} {model}")


@pytest.mark.parametrize("model", MODELS)
def test_maxit_2(model):
    want = G.reference("n257", model, maxit=2)
    assert (want["flags"] & G.MAXIT_BIT).any()
    compare(device_glm("n257", model, maxit=2), want, G.tolerance("n257", model, maxit=2), f"n257 {model} maxit 2")


@pytest.mark.parametrize("model", MODELS)
def test_prior_weights_with_zeros(model):
    assert (G.cohort(*G.CASES["n257"])[5] == 0).sum() == 2
    want = G.reference("n257", model, weighted=True)
    compare(device_glm("n257", model, weighted=True), want, G.tolerance("n257", model, weighted=True), f"n257 {model} weighted")


def test_genotype_with_an_empty_hom_class():
    """40 samples over 6 alleles: the rare alleles have no homozygote, so their fits have the het dummy alone."""
    want = G.reference("n40", "genotype", weighted=True)
    only_het = np.isfinite(want["coef"][:-1, 1]) & np.isnan(want["coef"][:-1, 2]) & (want["flags"][:-1] == 0)
    assert only_het.any()
    got = device_glm("n40", "genotype", weighted=True)
    compare(got, want, G.tolerance("n40", "genotype", weighted=True), "n40 genotype weighted")
    assert np.isfinite(got[0][:-1, 1][only_het]).all() and np.isnan(got[0][:-1, 2][only_het]).all()


# 2 feature rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_feature_rows_equal_the_restatement(model):
    n, n_allele, q, seed, part = G.CASES["n1000"]
    a1, a2, y, g, _, _ = G.cohort(n, n_allele, q, seed, part)
    A = AR.Analysis(a1, a2, y, n_allele, g, model)
    with assocglm._DeviceGlm(a1, a2, y, n_allele, g, MODELS.index(model)) as dev:
        rows = len(A.F)
        got = dev.feature_rows(0, rows)
        assert got.dtype == np.int8 and got.shape == (rows, A.n)
        assert got.tobytes() == A.F.astype(np.int8).tobytes()
        assert np.array_equal(dev.feature_rows(3, 2), A.F[3:5]) and dev.feature_rows(rows, 0).shape == (0, A.n)
        L = _lib.lib()
        out = np.empty((2, A.n), np.int8)
        for row0, k in ((-1, 1), (rows, 1), (rows - 1, 2), (0, -1)):
            assert L.hibag_hip_assoc_feature_rows(dev._h, row0, k, assoc._ptr(out)) == -1
        assert L.hibag_hip_assoc_feature_rows(dev._h, 0, 1, None) == -1 and L.hibag_hip_assoc_feature_rows(None, 0, 1, assoc._ptr(out)) == -1
        assert L.hibag_hip_assoc_n_kept(None) == -1


# 3 end to end ----------------------------------------------------------------------------------------------------
def assert_results_close(got, want, tol):
    assert got.name == want.name and np.array_equal(got.flags, want.flags)
    assert (got.n_samp, got.n_case, got.n_excluded) == (want.n_samp, want.n_case, want.n_excluded)
    ok = (want.flags & 2) == 0
    assert ok.sum() >= 10 and np.array_equal(got.iterations[ok], want.iterations[ok])
    for key in ("est", "se", "lower", "upper", "pval", "deviance", "lrt_stat", "lrt_p"):
        g, w = getattr(got, key), getattr(want, key)
        assert np.array_equal(np.isnan(g), np.isnan(w)), key
    scale = np.fmax(np.abs(want.est), want.se)
    assert np.nanmax(np.abs(got.est - want.est) / scale) <= tol and np.nanmax(np.abs(got.se / want.se - 1)) <= tol
    assert np.nanmax(np.abs(got.deviance / want.deviance - 1)) <= tol
    # what follows on the host: the bounds from est and se; z = est / se moves by 2 tol (1 + |z|), the p-values with it
    assert np.nanmax(np.abs(got.lower - want.lower) / scale) <= 3 * tol and np.nanmax(np.abs(got.upper - want.upper) / scale) <= 3 * tol
    z = np.abs(want.est / want.se)
    fin = np.isfinite(z)
    assert (np.abs(np.log(got.pval[fin] / want.pval[fin])) <= 4 * tol * (1 + z[fin]) ** 2 + 1e-12).all()
    dev_scale = tol * (np.abs(want.deviance) + abs(want.base["deviance"]))
    fin = np.isfinite(want.lrt_stat)
    assert (np.abs(got.lrt_stat - want.lrt_stat)[fin] <= dev_scale[fin]).all()
    small = fin & (want.lrt_stat > 1e-3)                                       # (the tail's log-derivative in the statistic is at most ~ 1 / stat + 1 / 2)
    assert (np.abs(np.log(got.lrt_p[small] / want.lrt_p[small])) <= dev_scale[small] * (1 / want.lrt_stat[small] + 1) + 1e-12).all()
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]
    b = np.fmax(np.abs(want.base["est"]), want.base["se"])
    assert (np.abs(got.base["est"] - want.base["est"]) <= tol * b).all() and (np.abs(got.base["se"] / want.base["se"] - 1) <= tol).all()


def test_hla_assoc_glm_end_to_end_and_conditioned():
    hla, y, groups, covar = G.hla_of("n1000")
    tol = G.tolerance("n1000", "dominant")
    want = hb.hlaAssocGlm(hla, y, covar, groups=groups, _backend=G.Backend)
    got = hb.hlaAssocGlm(hla, y, covar, groups=groups)
    assert_results_close(got, want, tol)
    assert got.flags[-1] == 2 and got.name[-1] == "pos:beyond"                  # a level the device does not know
    top = got.name[int(np.nanargmin(got.pval[:, 0]))]
    assert top == want.name[int(np.nanargmin(want.pval[:, 0]))]
    cwant = hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=[top], show_or=True, _backend=G.Backend)
    cgot = hb.hlaAssocGlm(hla, y, covar, groups=groups, condition=[top], show_or=True)
    assert cgot.flags[got.name.index(top)] & 2 and cgot.base["name"][-1] == f"h[{top}]"
    # (odds ratios: compared as logs)
    for r in (cgot, cwant):
        r.est, r.lower, r.upper = np.log(r.est), np.log(r.lower), np.log(r.upper)
    assert_results_close(cgot, cwant, tol)
    # the genotype model with prior weights
    hla, y, groups, covar = G.hla_of("n257")
    assert_results_close(hb.hlaAssocGlm(hla, y, covar, model="genotype", use_prob=True),
                         hb.hlaAssocGlm(hla, y, covar, model="genotype", use_prob=True, _backend=G.Backend),
                         G.tolerance("n257", "genotype", weighted=True))


# 4 reproducibility -----------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["dominant", "genotype"])
def test_results_are_bit_equal(model):
    """The same call twice; a handle with the alleles alone against one with the partition's tests beside them; before and
    after a permutation call on the handle (the kept labels survive it)."""
    first = device_glm("n1000", model)
    assert bits_equal(first, device_glm("n1000", model))
    n_allele = G.CASES["n1000"][1]
    alone = device_glm("n1000", model, alleles_only=True)
    assert len(alone[2]) == n_allele + 1 and len(first[2]) > n_allele + 1
    pick = list(range(n_allele)) + [-1]
    assert bits_equal(alone, [a[pick] for a in first])
    before, after = device_glm("n1000", model, permute_first=True)
    assert bits_equal(before, first) and bits_equal(after, first)


# 5 errors --------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0], np.int32)
    b = np.array([0, 0, 1, 1, 0, 1], np.int32)
    y = np.array([0, 1, 0, 1, 1, 0], np.int32)
    with assocglm._DeviceGlm(a, b, y, 2, None, 0) as dev:
        n_fit = dev.n_tests + 1
        coef, se = np.empty((n_fit, 16)), np.empty((n_fit, 16))
        d, it, fl = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        cov = np.arange(13 * 6, dtype=np.float64).reshape(13, 6) % 5
        w = np.ones(6)
        outs = (p(coef), p(se), p(d), p(it), p(fl))
        assert L.hibag_hip_assoc_glm(dev._h, p(cov), 1, p(w), 25, 1e-8, *outs) == 0 and np.isfinite(d[-1])
        assert L.hibag_hip_assoc_glm(dev._h, None, 0, None, 25, 1e-8, *outs) == 0
        assert L.hibag_hip_assoc_glm(dev._h, p(cov), 13, None, 25, 1e-8, *outs) == -1 and b"13 covariates" in L.hibag_hip_last_error()
        assert L.hibag_hip_assoc_glm(dev._h, p(cov), -1, None, 25, 1e-8, *outs) == -1
        assert L.hibag_hip_assoc_glm(dev._h, None, 1, None, 25, 1e-8, *outs) == -1
        assert L.hibag_hip_assoc_glm(dev._h, p(cov), 1, None, 0, 1e-8, *outs) == -1 and b"maxit" in L.hibag_hip_last_error()
        for eps in (0.0, -1.0, float("nan")):
            assert L.hibag_hip_assoc_glm(dev._h, p(cov), 1, None, 25, eps, *outs) == -1 and b"epsilon" in L.hibag_hip_last_error()
        bad = cov.copy()
        bad[1, 2] = np.nan
        assert L.hibag_hip_assoc_glm(dev._h, p(bad), 2, None, 25, 1e-8, *outs) == -1 and b"not finite" in L.hibag_hip_last_error()
        assert L.hibag_hip_assoc_glm(dev._h, p(bad), 1, None, 25, 1e-8, *outs) == 0       # (the first row alone is fine)
        for v in (-1.0, np.nan, np.inf):
            w2 = w.copy()
            w2[4] = v
            assert L.hibag_hip_assoc_glm(dev._h, p(cov), 1, p(w2), 25, 1e-8, *outs) == -1 and b"weight" in L.hibag_hip_last_error()
        for k in range(5):
            o = list(outs)
            o[k] = None
            assert L.hibag_hip_assoc_glm(dev._h, p(cov), 1, None, 25, 1e-8, *o) == -1
        assert L.hibag_hip_assoc_glm(None, p(cov), 1, None, 25, 1e-8, *outs) == -1
        assert b"hibag_hip_assoc_glm" in L.hibag_hip_last_error()
