"""hlaAssocOmnibus on the GPU: hibag_hip_assoc_glm_sets against the restatement (tests/assocomni_reference.py: DESIGN.md
section 26 in numpy) -- flags, iterations, degrees of freedom and the NaN pattern equal, estimates, standard errors and
deviances within a tolerance computed from the restatement alone (100 x its float64-versus-longdouble difference over the
run's fits, at least 1e-12: section 23's rule) --, at 40 / 255 / 256 / 257 / 1000 kept samples, for partitions of 2, 3, 5 and
8 levels, designs of 15, 16, 17 and 31 columns, no covariate and 29, sets too wide, empty, with a row nobody carries and
with an exactly aliased row, the three models, maxit = 2 and prior weights with zeros; one-row sets and the base model
against hibag_hip_assoc_glm; results bit-equal across calls, across the other sets of a call with the same H, and a
permutation call in between; invalid arguments rejected; hlaAssocOmnibus and hlaAssocStepwise end to end.

Measured: the largest device difference is 1.0 % of the tolerance (hlaAssocOmnibus conditioned on a
partition, 1000 kept samples: 1.0e-14 against the floor of 1e-12; among the runs of sets 0.94 %, n257 with maxit = 2); in the
run with the largest tolerance (n257 recessive, 12 covariates, fits of 15 iterations: 1.0e-8) the device is within 9.6e-12."""
import numpy as np
import pytest

import hibag_amd as hb
import assocglm_reference as G
import assocomni_reference as O
from hibag_amd import _lib, assoc, assocglm, assocomni

pytestmark = pytest.mark.gpu

MODELS = O.MODELS


def handle(case, model):
    n, n_allele, seed, extra = O.CASES[case]
    a1, a2, y, g, _, _ = O.cohort(n, n_allele, seed, extra)
    return assocomni._DeviceOmni(a1, a2, y, n_allele, g, MODELS.index(model))


def device_sets(case, model, q, weighted=False, maxit=25, sets=None, permute_between=False):
    A, covar, prob, _ = O.analysis(case, model)
    sets = O.run_sets(case, model, q) if sets is None else sets
    with handle(case, model) as dev:
        assert dev.n_kept == A.n
        got = dev.glm_sets(sets, covar[:q], prob if weighted else None, maxit, 1e-8)
        if permute_between:
            dev.permute(11, 1, 300)
            return got, dev.glm_sets(sets, covar[:q], prob if weighted else None, maxit, 1e-8)
        return got


def as_dict(got):
    return dict(zip(("coef", "se", "deviance", "iterations", "flags", "df_h"), got))


def compare(got, want, tol, what):
    """Section 23's comparison with section 26's additions: flags, iterations, df_h and the NaN pattern equal; the fits without
    the rank bit within tol; the others NaN."""
    got = as_dict(got)
    assert np.array_equal(got["flags"], want["flags"]), (what, got["flags"], want["flags"])
    fitted = (want["flags"] & O.RANK_BIT) == 0
    assert np.array_equal(got["iterations"][fitted], want["iterations"][fitted]), (what, got["iterations"], want["iterations"])
    assert np.array_equal(got["df_h"], want["df_h"]), (what, got["df_h"], want["df_h"])
    for k in ("coef", "se", "deviance"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k)
    assert np.isnan(got["deviance"][~fitted]).all() and np.isnan(got["coef"][~fitted]).all() and np.isnan(got["se"][~fitted]).all(), what
    d_est, d_se, d_dev = O.gaps(got, want)
    print(f"{what}: tol {tol:.3g}, device differences est {d_est:.3g} se {d_se:.3g} deviance {d_dev:.3g} "
          f"({max(d_est, d_se, d_dev) / tol:.3g} of tol), {int(fitted.sum())} fits, at most {int(got['iterations'].max())} iterations")
    assert d_est <= tol and d_se <= tol and d_dev <= tol, what


# 1 values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", O.DEVICE_RUNS, ids=lambda r: f"{r[0]}-{r[1]}-q{r[2]}" + ("-w" if r[3] else "") + (f"-maxit{r[4]}" if r[4] != 25 else ""))
def test_fits_equal_the_restatement(run):
    case, model, q, weighted, maxit = run
    want = O.reference(*run)
    assert ((want["flags"] & O.RANK_BIT) == 0).sum() >= 3
    compare(device_sets(case, model, q, weighted, maxit), want, O.tolerance(*run), f"{case} {model} q={q} weighted={weighted} maxit={maxit}")


def test_row_sums():
    A = O.analysis("n1000", "additive")[0]
    with handle("n1000", "additive") as dev:
        got = dev.row_sums()
        assert got.dtype == np.int32 and np.array_equal(got, A.rsum)
        assert np.array_equal(dev.feature_rows(0, len(A.F)).astype(np.int64).sum(axis=1), got)


# 2 against the 16-slot entry -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["additive", "dominant"])
def test_one_row_sets_equal_the_old_entry(model):
    """Every test of the handle as a set of one row, and the base model, against hibag_hip_assoc_glm's own numbers: the same
    fit but for the order of the factorisation (the covariates before the row), within the run's tolerance."""
    case, q = "n257", 12
    A, covar, _, _ = O.analysis(case, model)
    with handle(case, model) as dev:
        coef, se, dev_t, it, fl = dev.glm(covar[:q], None, 25, 1e-8)
        ok = np.flatnonzero((fl[:-1] & G.RANK_BIT) == 0)
        assert len(ok) >= 20
        sets = [[int(t)] for t in ok]
        got = as_dict(dev.glm_sets(sets, covar[:q], None, 25, 1e-8))
    r, rl = (O.glm_sets(A.F, sets, covar[:q], None, A.y, dtype=d) for d in (np.float64, np.longdouble))
    tol = max(100.0 * max(O.gaps(r, rl)), 1e-12)
    pick = list(ok) + [len(fl) - 1]
    old_slots = [0, 1] + list(range(G.COV0, G.COV0 + q))
    new_slots = [0, 1] + list(range(2, 2 + q))
    want = dict(coef=np.full((len(pick), 32), np.nan), se=np.full((len(pick), 32), np.nan), deviance=dev_t[pick],
                flags=fl[pick])
    want["coef"][:, new_slots], want["se"][:, new_slots] = coef[pick][:, old_slots], se[pick][:, old_slots]
    assert np.array_equal(got["flags"], fl[pick]) and np.array_equal(got["iterations"], it[pick])
    assert np.array_equal(got["df_h"], [1] * len(ok) + [0])
    assert np.array_equal(np.isnan(got["coef"]), np.isnan(want["coef"]))
    d = O.gaps(got, want)
    print(f"one-row sets, {model}: tol {tol:.3g}, differences est {d[0]:.3g} se {d[1]:.3g} deviance {d[2]:.3g} ({max(d) / tol:.3g} of tol)")
    assert max(d) <= tol


# 3 reproducibility -----------------------------------------------------------------------------------------------
def bits_equal(a, b, rows_a=None, rows_b=None):
    return all(x[rows_a if rows_a is not None else slice(None)].tobytes() == y[rows_b if rows_b is not None else slice(None)].tobytes()
               for x, y in zip(a, b))


def test_results_are_bit_equal():
    """The same call twice and after a permutation call on the handle; a set alone, and with one other, against the same set
    among all the run's sets, H being the same in the three calls (the largest fitted set is in each of them)."""
    case, model, q = "n1000", "additive", 6
    sets = O.run_sets(case, model, q)
    first, second = device_sets(case, model, q, permute_between=True)
    assert bits_equal(first, second) and bits_equal(first, device_sets(case, model, q))
    want = O.reference(case, model, q)
    big = max((i for i in range(len(sets)) if not want["flags"][i] & O.RANK_BIT), key=lambda i: len(sets[i]))
    assert len(sets[big]) == want["H"] == 24
    alone = device_sets(case, model, q, sets=[sets[big]])
    assert bits_equal(alone, first, [0, 1], [big, len(sets)])
    pair = device_sets(case, model, q, sets=[sets[2], sets[big]])
    assert bits_equal(pair, first, [0, 1, 2], [2, big, len(sets)])
    assert np.isfinite(first[0][2, 1:5]).all()


# 4 errors --------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0, 2, 2], np.int32)
    b = np.array([0, 0, 1, 1, 2, 1, 0, 2], np.int32)
    y = np.array([0, 1, 0, 1, 1, 0, 1, 0], np.int32)
    with assocomni._DeviceOmni(a, b, y, 3, None, 1) as dev:
        n_fit = 3
        coef, se = np.empty((n_fit, 32)), np.empty((n_fit, 32))
        d, it, fl, df = np.empty(n_fit), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32), np.empty(n_fit, np.int32)
        cov = np.arange(30 * 8, dtype=np.float64).reshape(30, 8) % 5
        w = np.ones(8)
        start, rows = np.array([0, 1, 3], np.int32), np.array([1, 1, 2], np.int32)
        outs = (p(coef), p(se), p(d), p(it), p(fl), p(df))

        def call(start=start, rows=rows, n_sets=2, cov=cov, q=1, w=None, maxit=25, eps=1e-8, outs=outs, h=dev._h):
            return L.hibag_hip_assoc_glm_sets(h, p(start), p(rows), n_sets, p(cov), q, p(w), maxit, eps, *outs)

        assert call() == 0 and np.isfinite(d[-1]) and fl[-1] == 0 and df.tolist()[2] == 0
        assert call(w=w) == 0 and call(cov=None, q=0) == 0 and call(n_sets=0) == 0
        assert call(q=30) == -1 and b"30 covariates" in L.hibag_hip_last_error()
        assert call(q=-1) == -1 and call(cov=None, q=1) == -1
        assert call(maxit=0) == -1 and b"maxit" in L.hibag_hip_last_error()
        for eps in (0.0, -1.0, float("nan")):
            assert call(eps=eps) == -1 and b"epsilon" in L.hibag_hip_last_error()
        bad = cov.copy()
        bad[1, 2] = np.nan
        assert call(cov=bad, q=2) == -1 and b"not finite" in L.hibag_hip_last_error()
        assert call(cov=bad, q=1) == 0                                          # (the first row alone is fine)
        for v in (-1.0, np.nan, np.inf):
            w2 = w.copy()
            w2[4] = v
            assert call(w=w2) == -1 and b"weight" in L.hibag_hip_last_error()
        for k in range(6):
            o = list(outs)
            o[k] = None
            assert call(outs=o) == -1
        assert call(h=None) == -1 and b"hibag_hip_assoc_glm_sets" in L.hibag_hip_last_error()
        # the sets
        assert call(start=None) == -1 and call(n_sets=-1) == -1
        assert call(start=np.array([1, 1, 3], np.int32)) == -1 and b"set_start" in L.hibag_hip_last_error()
        assert call(start=np.array([0, 2, 1], np.int32)) == -1 and b"monotone" in L.hibag_hip_last_error()
        assert call(rows=None) == -1 and b"set_rows" in L.hibag_hip_last_error()
        assert call(rows=np.array([1, 1, 3], np.int32)) == -1 and b"outside" in L.hibag_hip_last_error()
        assert call(rows=np.array([-1, 1, 2], np.int32)) == -1 and b"outside" in L.hibag_hip_last_error()
        assert call(rows=np.array([1, 2, 2], np.int32)) == -1 and b"twice" in L.hibag_hip_last_error()
        assert call(rows=np.array([2, 2, 1], np.int32)) == 0                    # (the same row in two sets is fine)
        assert L.hibag_hip_assoc_row_sums(None, p(df)) == -1 and L.hibag_hip_assoc_row_sums(dev._h, None) == -1


# 5 end to end ----------------------------------------------------------------------------------------------------
class LongBackend(O.Backend):
    dtype = np.longdouble


def assert_results_close(got, want, long):
    """The device's result against the restatement's, with the tolerance of these very fits: 100 x the restatement's own
    float64-versus-longdouble difference, at least 1e-12."""
    assert got.name == want.name and got.reference == want.reference and got.level_names == want.level_names
    for k in ("flags", "df", "iterations", "n_levels"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert (got.n_samp, got.n_case, got.n_excluded) == (want.n_samp, want.n_case, want.n_excluded)
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]

    def flat(r):
        est = np.concatenate(r.est + [r.base["est"]]).astype(np.float64)
        se = np.concatenate(r.se + [r.base["se"]]).astype(np.float64)
        return est, se, np.append(r.deviance, r.base["deviance"]).astype(np.float64)

    (ge, gs, gd), (we, ws, wd), (le, ls, ld) = flat(got), flat(want), flat(long)
    assert np.array_equal(np.isnan(ge), np.isnan(we)) and np.array_equal(np.isnan(gs), np.isnan(ws)) and np.array_equal(np.isnan(gd), np.isnan(wd))
    scale = np.fmax(np.abs(we), ws)
    with np.errstate(invalid="ignore"):
        tol = max(100.0 * max(np.nanmax(np.abs(we - le) / scale), np.nanmax(np.abs(ws / ls - 1)), np.nanmax(np.abs(wd / ld - 1))), 1e-12)
        share = max(np.nanmax(np.abs(ge - we) / scale), np.nanmax(np.abs(gs / ws - 1)), np.nanmax(np.abs(gd / wd - 1))) / tol
    print(f"end to end: tol {tol:.3g}, the device at {share:.3g} of it")
    assert share <= 1.0
    for k in ("lower", "upper", "pval"):
        for g, w in zip(getattr(got, k), getattr(want, k)):
            assert np.array_equal(np.isnan(g), np.isnan(w)), k
    for g, w, e, s in zip(got.lower + got.upper, want.lower + want.upper, want.est * 2, want.se * 2):
        with np.errstate(invalid="ignore"):
            assert not (np.abs(g - w) > 3 * tol * np.fmax(np.abs(e), s)).any()
    assert np.array_equal(np.isnan(got.lrt_stat), np.isnan(want.lrt_stat)) and np.array_equal(np.isnan(got.lrt_p), np.isnan(want.lrt_p))
    dev_scale = tol * (np.abs(want.deviance) + abs(want.base["deviance"]))
    fin = np.isfinite(want.lrt_stat)
    assert fin.sum() >= 3 and (np.abs(got.lrt_stat - want.lrt_stat)[fin] <= dev_scale[fin]).all()
    small = np.isfinite(want.lrt_p) & (want.lrt_stat > 1e-3)   # (the tail's log-derivative in the statistic is at most ~ 1 / stat + 1 / 2)
    assert (np.abs(np.log(got.lrt_p[small] / want.lrt_p[small])) <= dev_scale[small] * (1 / want.lrt_stat[small] + 1) + 1e-12).all()


def test_hla_assoc_omnibus_end_to_end_and_conditioned():
    hla, y, groups, covar = O.hla_of("n1000")
    covar = covar[:, :6]
    for kw in ({}, {"condition": ["p3"]}, {"model": "dominant", "use_prob": True, "condition": ["p2", "03:01"]}):
        got = hb.hlaAssocOmnibus(hla, y, groups, covar, **kw)
        want = hb.hlaAssocOmnibus(hla, y, groups, covar, _backend=O.Backend, **kw)
        assert_results_close(got, want, hb.hlaAssocOmnibus(hla, y, groups, covar, _backend=LongBackend, **kw))
        if kw.get("condition") == ["p3"]:
            for name in ("p3", "p3b"):                                       # the conditioned partition, and its copy
                i = got.name.index(name)
                assert got.df[i] == 0 and got.flags[i] & 8 and np.isnan(got.lrt_p[i]) and np.isnan(got.est[i]).all()
            assert got.base["name"][-2:] == ["h[p3:p3.1]", "h[p3:p3.2]"] and got.reference[got.name.index("p3")] == "p3.0"
            assert got.flags[got.name.index("all")] == 16 | 2                # (23 columns beside 8)


def test_hla_assoc_stepwise_end_to_end():
    hla, y, groups, covar = O.hla_of("n1000", without=("p3b",))
    got = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], p_stop=1e-6)
    want = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], p_stop=1e-6, _backend=O.Backend)
    assert got.chosen == want.chosen and got.chosen[0] == "p3" and len(got.steps) == len(want.steps) == len(got.chosen) + 1
    long = hb.hlaAssocStepwise(hla, y, groups, covar[:, :6], p_stop=1e-6, _backend=LongBackend)
    assert long.chosen == want.chosen
    for g, w, ld in zip(got.steps, want.steps, long.steps):
        assert_results_close(g, w, ld)
