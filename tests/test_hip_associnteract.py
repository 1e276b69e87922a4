"""hlaAssocInteract on the GPU: hibag_hip_assoc_row_gram against the integer products of the handle's own feature rows, exactly;
hibag_hip_assoc_glm_terms against the restatement (tests/associnteract_reference.py: DESIGN.md section 27 in numpy) -- flags,
iterations, degrees of freedom and the NaN pattern equal, estimates, standard errors and deviances within a tolerance computed
from the restatement alone (100 x its float64-versus-longdouble difference over the run's fits, at least 1e-12: section 23's
rule) --, at 40 / 255 / 256 / 257 / 1000 kept samples with 0 / 1 / 5 / 11 / 6 covariates, for fits of one, two and three terms,
plain rows and products, a product nobody carries beside carried main effects, an exactly aliased product, records with no
term, the three models, maxit = 2 and prior weights with zeros; plain-term fits and the base model against
hibag_hip_assoc_glm; a fit's results bit-equal alone, with one other fit, among all, across calls and a permutation call in
between; invalid arguments rejected by their messages; hlaAssocInteract end to end.

Measured: the largest device difference is 1.5 % of the tolerance (256 kept samples: est 1.5e-14 in units
of max(|est|, se) against the floor of 1e-12); in the run with the largest tolerance (n257 recessive, 11 covariates, fits of 15
iterations: 9.7e-9) the device is within 5.4e-12 (se); end to end 1.1 % (the default pairs at 257 kept samples, tol 2.2e-9)."""
import numpy as np
import pytest

import hibag_amd as hb
import assocglm_reference as G
import associnteract_reference as I
import assocomni_reference as O
from hibag_amd import _lib, assoc, associnteract

pytestmark = pytest.mark.gpu

OUT = ("coef", "se", "deviance", "iterations", "flags", "df_h")


def handle(case, model):
    n, n_allele, seed, extra = I.CASES[case]
    a1, a2, y, g, _, _ = O.cohort(n, n_allele, seed, extra)
    return associnteract._DeviceInteract(a1, a2, y, n_allele, g, assoc.MODELS.index(model))


def device_terms(case, model, q, weighted=False, maxit=25, fits=None, permute_between=False):
    A, covar, prob, _ = I.analysis(case, model)
    fits = I.run_fits(case, model) if fits is None else fits
    with handle(case, model) as dev:
        assert dev.n_kept == A.n
        got = dev.glm_terms(fits, covar[:q], prob if weighted else None, maxit, 1e-8)
        if permute_between:
            dev.permute(11, 1, 300)
            return got, dev.glm_terms(fits, covar[:q], prob if weighted else None, maxit, 1e-8)
        return got


def compare(got, want, tol, what):
    """Section 23's comparison with section 26's additions: flags, iterations, df_h and the NaN pattern equal; the fits without
    the rank bit within tol; the others NaN."""
    got = dict(zip(OUT, got))
    assert np.array_equal(got["flags"], want["flags"]), (what, got["flags"], want["flags"])
    fitted = (want["flags"] & I.RANK_BIT) == 0
    assert np.array_equal(got["iterations"], want["iterations"]), (what, got["iterations"], want["iterations"])   # (0 where not fitted)
    assert np.array_equal(got["df_h"], want["df_h"]), (what, got["df_h"], want["df_h"])
    for k in ("coef", "se", "deviance"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k)
    assert np.isnan(got["deviance"][~fitted]).all() and np.isnan(got["coef"][~fitted]).all() and np.isnan(got["se"][~fitted]).all(), what
    d_est, d_se, d_dev = I.gaps(got, want)
    print(f"{what}: tol {tol:.3g}, device differences est {d_est:.3g} se {d_se:.3g} deviance {d_dev:.3g} "
          f"({max(d_est, d_se, d_dev) / tol:.3g} of tol), {int(fitted.sum())} fits, at most {int(got['iterations'].max())} iterations")
    assert d_est <= tol and d_se <= tol and d_dev <= tol, what


# 1 the Gram ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["additive", "dominant"])
def test_row_gram_is_exact(model):
    """The whole handle (at 1000 kept samples more than 64 rows: more than one tile) and 65 rows from row 3 on."""
    with handle("n1000", model) as dev:
        F = dev.feature_rows(0, dev.n_rows).astype(np.int64)
        assert dev.n_rows > 64 + 3
        got = dev.row_gram(0, dev.n_rows)
        assert got.dtype == np.int32 and np.array_equal(got, F @ F.T)
        assert np.array_equal(dev.row_gram(3, 65), (F @ F.T)[3:68, 3:68])
        assert np.array_equal(dev.row_gram(dev.n_rows - 1, 1), (F @ F.T)[-1:, -1:]) and dev.row_gram(5, 0).shape == (0, 0)
        if model == "dominant":
            assert np.array_equal(np.diag(got), dev.row_sums())


# 2 values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", I.DEVICE_RUNS, ids=lambda r: f"{r[0]}-{r[1]}-q{r[2]}" + ("-w" if r[3] else "") + (f"-maxit{r[4]}" if r[4] != 25 else ""))
def test_fits_equal_the_restatement(run):
    case, model, q, weighted, maxit = run
    want, fits = I.reference(*run), I.run_fits(case, model)
    fitted = (want["flags"] & I.RANK_BIT) == 0
    assert fitted.sum() >= 3
    assert any(fits[f, 2, 1] >= 0 and np.isfinite(want["coef"][f, 3]) for f in range(len(fits)))        # an active product
    compare(device_terms(case, model, q, weighted, maxit), want, I.tolerance(*run), f"{case} {model} q={q} weighted={weighted} maxit={maxit}")


# 3 against the 16-slot entry of hlaAssocGlm -------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["additive", "dominant"])
def test_plain_terms_equal_the_old_entry(model):
    """Every test of the handle as a fit of one plain term, and the base model, against hibag_hip_assoc_glm's own numbers: the
    same fit but for the slot of the covariates and the order of the factorisation (the covariates before the term)."""
    case, q = "n257", 11
    A, covar, _, _ = I.analysis(case, model)
    with handle(case, model) as dev:
        coef, se, dev_t, it, fl = dev.glm(covar[:q], None, 25, 1e-8)
        ok = np.flatnonzero((fl[:-1] & G.RANK_BIT) == 0)
        assert len(ok) >= 20
        fits = np.array([[(int(t), -1), I.UNUSED, I.UNUSED] for t in ok], np.int32)
        got = dict(zip(OUT, dev.glm_terms(fits, covar[:q], None, 25, 1e-8)))
    tol = I.tolerance_of(*(I.glm_terms(A.F, fits, covar[:q], None, A.y, dtype=d) for d in (np.float64, np.longdouble)))
    pick = list(ok) + [len(fl) - 1]
    old_slots = [0, 1] + list(range(G.COV0, G.COV0 + q))
    new_slots = [0, 1] + list(range(I.COV0, I.COV0 + q))
    want = dict(coef=np.full((len(pick), 16), np.nan), se=np.full((len(pick), 16), np.nan), deviance=dev_t[pick], flags=fl[pick])
    want["coef"][:, new_slots], want["se"][:, new_slots] = coef[pick][:, old_slots], se[pick][:, old_slots]
    assert np.array_equal(got["flags"], fl[pick]) and np.array_equal(got["iterations"], it[pick])
    assert np.array_equal(got["df_h"], [1] * len(ok) + [0])
    assert np.array_equal(np.isnan(got["coef"]), np.isnan(want["coef"])) and np.array_equal(np.isnan(got["se"]), np.isnan(want["se"]))
    d = I.gaps(got, want)
    print(f"plain terms, {model}: tol {tol:.3g}, differences est {d[0]:.3g} se {d[1]:.3g} deviance {d[2]:.3g} ({max(d) / tol:.3g} of tol)")
    assert max(d) <= tol


# 4 reproducibility -----------------------------------------------------------------------------------------------
def bits_equal(a, b, rows_a, rows_b):
    return all(x[rows_a].tobytes() == y[rows_b].tobytes() for x, y in zip(a, b))


def test_results_are_bit_equal():
    """The same call twice and after a permutation call on the handle; a fit alone, and with one other, against the same
    fit among all the run's fits (the base model comes last in each call)."""
    case, model, q = "n1000", "additive", 6
    fits = I.run_fits(case, model)
    every = list(range(len(fits) + 1))
    first, second = device_terms(case, model, q, permute_between=True)
    assert bits_equal(first, second, every, every) and bits_equal(first, device_terms(case, model, q), every, every)
    for f in (1, 15, 19):                                                     # a full fit, three plain terms, levels and their product
        assert np.isfinite(first[0][f, 1:4]).all()
        alone = device_terms(case, model, q, fits=fits[[f]])
        assert bits_equal(alone, first, [0, 1], [f, len(fits)])
        pair = device_terms(case, model, q, fits=fits[[2, f]])
        assert bits_equal(pair, first, [0, 1, 2], [2, f, len(fits)])


# 5 errors --------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0, 2, 2], np.int32)
    b = np.array([0, 0, 1, 1, 2, 1, 0, 2], np.int32)
    y = np.array([0, 1, 0, 1, 1, 0, 1, 0], np.int32)
    with associnteract._DeviceInteract(a, b, y, 3, None, 1) as dev:
        n_fit = 3
        coef, se = np.empty((n_fit, 16)), np.empty((n_fit, 16))
        d, it, fl, df = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        cov = np.arange(12 * 8, dtype=np.float64).reshape(12, 8) % 5
        w = np.ones(8)
        terms = np.array([[(0, -1), (1, -1), (-1, -1)], [(0, -1), (1, -1), (0, 1)]], np.int32)
        outs = (p(coef), p(se), p(d), p(it), p(fl), p(df))
        err = L.hibag_hip_last_error

        def call(terms=terms, n_fits=2, cov=cov, q=1, w=None, maxit=25, eps=1e-8, outs=outs, h=dev._h):
            return L.hibag_hip_assoc_glm_terms(h, p(terms), n_fits, p(cov), q, p(w), maxit, eps, *outs)

        def with_term(f, j, pair):
            t = terms.copy()
            t[f, j] = pair
            return t

        assert call() == 0 and np.isfinite(d[-1]) and fl[-1] == 0 and df.tolist()[2] == 0
        assert call(w=w) == 0 and call(cov=None, q=0) == 0 and call(n_fits=0) == 0 and call(terms=None, n_fits=0) == 0
        assert call(q=12) == -1 and b"hibag_hip_assoc_glm_terms: 12 covariates; 0 .. 11" in err()
        assert call(q=-1) == -1 and b"-1 covariates" in err()
        assert call(cov=None, q=1) == -1 and b"with covar" in err()
        assert call(maxit=0) == -1 and b"hibag_hip_assoc_glm_terms: maxit" in err()
        for eps in (0.0, -1.0, float("nan")):
            assert call(eps=eps) == -1 and b"hibag_hip_assoc_glm_terms: epsilon" in err()
        bad = cov.copy()
        bad[1, 2] = np.nan
        assert call(cov=bad, q=2) == -1 and b"hibag_hip_assoc_glm_terms: covariate 1 of kept sample 2 is not finite" in err()
        assert call(cov=bad, q=1) == 0                                          # (the first row alone is fine)
        for v in (-1.0, np.nan, np.inf):
            w2 = w.copy()
            w2[4] = v
            assert call(w=w2) == -1 and b"hibag_hip_assoc_glm_terms: weight[4]" in err()
        for k in range(6):
            o = list(outs)
            o[k] = None
            assert call(outs=o) == -1 and b"hibag_hip_assoc_glm_terms: null argument" in err()
        assert call(h=None) == -1 and b"hibag_hip_assoc_glm_terms: null argument" in err()
        # the fit records
        assert call(n_fits=-1) == -1 and b"n_fits" in err()
        assert call(n_fits=(1 << 20) + 1) == -1 and b"n_fits" in err()
        assert call(terms=None) == -1 and b"terms with fits to read" in err()
        for pair in ((3, -1), (0, 3), (-2, -1), (0, -2)):
            assert call(terms=with_term(1, 2, pair)) == -1 and b"outside the handle's 3" in err()
        assert call(terms=with_term(0, 2, (-1, 2))) == -1 and b"row_a = -1 with row_b = 2" in err()
        assert call(terms=with_term(0, 2, (1, -1))) == -1 and b"twice" in err()
        assert call(terms=with_term(1, 1, (1, 0))) == -1 and b"twice" in err()    # (1, 0) is (0, 1)
        assert call(terms=with_term(1, 1, (2, 2))) == 0                          # (a row with itself is a term like any other)
        assert call(terms=with_term(0, 0, (-1, -1))) == 0                        # (unused slots may repeat)
        # the Gram
        out = np.empty((3, 3), np.int32)
        G3 = L.hibag_hip_assoc_row_gram
        assert G3(dev._h, 0, 3, p(out)) == 0 and G3(dev._h, 3, 0, None) == 0
        assert G3(None, 0, 3, p(out)) == -1 and b"hibag_hip_assoc_row_gram: null" in err()
        assert G3(dev._h, 0, 3, None) == -1 and b"hibag_hip_assoc_row_gram: null" in err()
        assert G3(dev._h, 0, -1, p(out)) == -1 and b"hibag_hip_assoc_row_gram" in err()
        for row0, n_rows in ((-1, 2), (1, 3), (4, 0)):
            assert G3(dev._h, row0, n_rows, p(out)) == -1 and b"hibag_hip_assoc_row_gram: rows" in err()
    # more rows than a call takes: a handle with 8200 tests (one partition of 8197 levels, all but three of them empty)
    g = np.array([[0, 1, 8196]], np.int32)
    with associnteract._DeviceInteract(a, b, y, 3, g, 1) as dev:
        assert dev.n_rows == 8200
        big = np.empty(1, np.int32)
        assert L.hibag_hip_assoc_row_gram(dev._h, 0, 8193, p(big)) == -1 and b"hibag_hip_assoc_row_gram: 8193 rows; at most 8192" in err()


# 6 end to end ----------------------------------------------------------------------------------------------------
class LongBackend(I.Backend):
    dtype = np.longdouble


def assert_results_close(got, want, long):
    """The device's result against the restatement's, with the tolerance of these very fits: 100 x the restatement's own
    float64-versus-longdouble difference, at least 1e-12 (as assert_results_close of tests/test_hip_assocomni.py)."""
    assert (got.name_a, got.name_b) == (want.name_a, want.name_b) and np.array_equal(got.both, want.both)
    for k in ("flags_main", "flags_full", "iterations_main", "iterations_full", "df_main", "df_full"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert (got.n_samp, got.n_case, got.n_excluded) == (want.n_samp, want.n_case, want.n_excluded)
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]

    def flat(r):
        est = np.concatenate([r.est.ravel(), r.base["est"]]).astype(np.float64)
        se = np.concatenate([r.se.ravel(), r.base["se"]]).astype(np.float64)
        return est, se, np.concatenate([r.deviance_main, r.deviance_full, [r.base["deviance"]]]).astype(np.float64)

    (ge, gs, gd), (we, ws, wd), (le, ls, ld) = flat(got), flat(want), flat(long)
    assert np.array_equal(np.isnan(ge), np.isnan(we)) and np.array_equal(np.isnan(gs), np.isnan(ws)) and np.array_equal(np.isnan(gd), np.isnan(wd))
    scale = np.fmax(np.abs(we), ws)
    with np.errstate(invalid="ignore"):
        tol = max(100.0 * max(np.nanmax(np.abs(we - le) / scale), np.nanmax(np.abs(ws / ls - 1)), np.nanmax(np.abs(wd / ld - 1))), 1e-12)
        share = max(np.nanmax(np.abs(ge - we) / scale), np.nanmax(np.abs(gs / ws - 1)), np.nanmax(np.abs(gd / wd - 1))) / tol
    print(f"end to end: tol {tol:.3g}, the device at {share:.3g} of it")
    assert share <= 1.0
    for k in ("lower", "upper", "pval"):
        assert np.array_equal(np.isnan(getattr(got, k)), np.isnan(getattr(want, k))), k
    for g, w in ((got.lower, want.lower), (got.upper, want.upper)):
        with np.errstate(invalid="ignore"):
            assert not (np.abs(g - w) > 3 * tol * np.fmax(np.abs(want.est), want.se)).any()
    assert np.array_equal(np.isnan(got.lrt_stat), np.isnan(want.lrt_stat)) and np.array_equal(np.isnan(got.lrt_p), np.isnan(want.lrt_p))
    dev_scale = tol * (np.abs(want.deviance_main) + np.abs(want.deviance_full))
    fin = np.isfinite(want.lrt_stat)
    assert fin.sum() >= 3 and (np.abs(got.lrt_stat - want.lrt_stat)[fin] <= dev_scale[fin]).all()
    small = np.isfinite(want.lrt_p) & (want.lrt_stat > 1e-3)   # (the tail's log-derivative in the statistic is at most ~ 1 / stat + 1 / 2)
    assert small.sum() >= 3
    assert (np.abs(np.log(got.lrt_p[small] / want.lrt_p[small])) <= dev_scale[small] * (1 / want.lrt_stat[small] + 1) + 1e-12).all()


@pytest.mark.parametrize("which", [0, 1], ids=["default-pairs", "explicit-pairs"])
def test_hla_assoc_interact_end_to_end(which):
    case, q, kw = I.END_TO_END[which]
    hla, y, groups, covar = I.hla_of(case)
    covar = covar[:, :q]
    got = hb.hlaAssocInteract(hla, y, covar, groups=groups, **kw)
    want = hb.hlaAssocInteract(hla, y, covar, groups=groups, _backend=I.Backend, **kw)
    assert_results_close(got, want, hb.hlaAssocInteract(hla, y, covar, groups=groups, _backend=LongBackend, **kw))
    if which == 1:
        assert got.flags_full[5] & I.ALIASED_BIT and np.isnan(got.est[5, 2]) and np.isnan(got.lrt_p[5])     # 01:01 x p2.0 = 01:01
        assert got.both[6] == 0 and got.flags_full[6] == I.RANK_BIT and np.isnan(got.deviance_full[6])      # below min_both
        assert got.base["name"][-1] == "h[03:01]"
