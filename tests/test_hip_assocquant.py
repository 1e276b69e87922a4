"""hlaAssocQuant on the GPU: the hibag_hip_assoc_quant_* entries against the restatement (tests/assocquant_reference.py:
DESIGN.md section 25 in numpy) -- the permutation rows byte for byte; class counts, flags and permutation counts equal as
integers; the class sums, projections, Gram cells, rr, statistics and per-permutation maxima within a tolerance computed
from the restatement alone (100 x its float64-versus-longdouble difference over the case, at least 1e-12; each quantity in
units of its own scale, ``assocquant_reference.differences``) --, at cohort sizes around the 128-sample padding and the
16-row tiles, for the four models and 1 .. 200 permutations; results bit-equal across panel sizes, split calls, handles with
more tests, repeated calls and other entries' calls in between; hlaAssocQuant end to end; invalid arguments rejected.

The integer comparisons of the counts rest on the safety condition that tests/test_assocquant_host.py asserts for every
case here: no permuted statistic within 1e-6 relative of its observed one.

Measured: the largest device difference is 34 % of its case's tolerance (n1000: S2 3.4e-13 relative
against 1e-12); g within 1.1e-16 of sqrt(xx rr), stat and max_stat within 9.0e-15 of max(|T|, 1)."""
import numpy as np
import pytest

import hibag_amd as hb
import assocquant_reference as Q
from hibag_amd import _lib, assoc, assocquant

pytestmark = pytest.mark.gpu

MODELS = Q.MODELS


def open_case(case, model, alleles_only=False):
    n, n_allele, q, seed, n_na, part = Q.CASES[case]
    a1, a2, y, g, covar = Q.cohort(n, n_allele, q, seed, n_na, part)
    yk, ck = Q.kept_columns(a1, a2, y, covar)
    dev = assocquant._DeviceQuant(a1, a2, np.zeros(n, np.int32), n_allele, None if alleles_only else g, MODELS.index(model))
    assert dev.n_kept == n - n_na
    dev.quant(yk, ck)
    return dev


def device_numbers(dev, Z, n_perm, seed):
    cnt, S1, S2, ybar = dev.quant_classes()
    proj, g, rr, stat, flags = dev.quant_observed()
    max_stat, count = dev.quant_permute(seed, 1, n_perm)
    return dict(cnt=cnt, S1=S1, S2=S2, proj=proj, g=g, rr=rr, stat=stat, max_stat=max_stat), ybar, flags, count


# 1 the generator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n5", "n257"])
def test_perm_rows_byte_for_byte(case):
    with open_case(case, "dominant") as dev:
        n = dev.n_kept
        for rows, seed, perm0 in ((1, 0, 1), (2, 0xFFFFFFFFFFFFFFFF, (1 << 64) - 3), (127, 0x0123456789ABCDEF, (1 << 40) + 7),
                                  (128, 1 << 32, (1 << 32) - 64), (129, 0x9E3779B97F4A7C15, 1 << 63), (300, 12345, 1)):
            got = dev.quant_perm_rows(seed, perm0, rows)
            want = Q.perm_rows(seed, perm0, rows, n)
            assert got.dtype == np.int32 and got.shape == (rows, n)
            assert got.tobytes() == want.tobytes(), (case, rows, seed, perm0)
        assert dev.quant_perm_rows(3, 5, 0).shape == (0, n)


def test_perm_rows_across_panels(monkeypatch):
    """40 rows in panels of 16, 16 and 8: each panel reaches the host before the next overwrites the device's buffer."""
    monkeypatch.setenv("HIBAG_QUANT_PANEL_PERMS", "16")
    with open_case("n40", "dominant") as dev:
        seed = Q.seed_of("n40", "dominant")
        assert dev.quant_perm_rows(seed, 1, 40).tobytes() == Q.perm_rows(seed, 1, 40, dev.n_kept).tobytes()


# 2 values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(Q.CASES))
def test_numbers_equal_the_restatement(case, model):
    Z = Q.reference(case, model)
    tol = Q.tolerance(case, model)
    want = Q.numbers(Z)
    with open_case(case, model) as dev:
        assert dev.n_tests == Z.T
        for n_perm in Q.PERM_COUNTS[case]:
            got, ybar, flags, count = device_numbers(dev, Z, n_perm, Z.seed)
            assert got["cnt"].dtype == np.int64 and np.array_equal(got["cnt"], Z.cnt)
            assert np.array_equal(flags, Z.flags), (flags, Z.flags)
            assert abs(ybar - float(Z.ybar)) <= tol * abs(float(Z.ybar))
            for key in ("proj", "g", "stat"):
                assert np.array_equal(np.isnan(got[key]), np.isnan(np.asarray(want[key], np.float64))), key
            assert np.isnan(got["stat"][Z.flags != 0]).all()
            w = dict(want, max_stat=Z.max_stat[:n_perm])
            d = Q.differences(got, w)
            print(f"{case} {model} {n_perm} permutations: tol {tol:.3g}, device differences " +
                  " ".join(f"{k} {v:.3g}" for k, v in d.items()) + f" ({max(d.values()) / tol:.3g} of tol)")
            assert max(d.values()) <= tol, d
            with np.errstate(invalid="ignore"):
                want_count = (Z.perm_T[:, :n_perm] >= Z.stat[:, None]).sum(axis=1)
            assert count.dtype == np.int64 and np.array_equal(count, want_count), (count, want_count)


# 3 reproducibility --------------------------------------------------------------------------------------------------------
def all_bits(dev, seed, n_perm):
    out = list(dev.quant_classes()) + list(dev.quant_observed()) + list(dev.quant_permute(seed, 1, n_perm))
    return [np.asarray(a) for a in out]


def bits_equal(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["dominant", "genotype"])
def test_results_are_bit_equal(model, monkeypatch):
    """Panels of 16 against the default; two calls of 100 against one of 200; the same call twice; the alleles alone
    against the alleles with the partition's tests beside them; before and after a permutation call and a regression call of
    the other entries on the same handle."""
    seed = 0xC0FFEE1234567890
    n_allele = Q.CASES["n1000"][1]
    with open_case("n1000", model) as dev:
        first = all_bits(dev, seed, 200)
        assert bits_equal(first, all_bits(dev, seed, 200))
        monkeypatch.setenv("HIBAG_QUANT_PANEL_PERMS", "16")
        assert bits_equal(first, all_bits(dev, seed, 200))
        monkeypatch.setenv("HIBAG_QUANT_PANEL_PERMS", "48")                       # (a last panel of 8: half a tile)
        assert bits_equal(first, all_bits(dev, seed, 200))
        monkeypatch.delenv("HIBAG_QUANT_PANEL_PERMS")
        m1, c1 = dev.quant_permute(seed, 1, 100)
        m2, c2 = dev.quant_permute(seed, 101, 100)
        assert np.concatenate([m1, m2]).tobytes() == first[-2].tobytes() and np.array_equal(c1 + c2, first[-1])
        dev.permute(11, 1, 300)
        dev.glm(None, None, 25, 1e-8)
        assert bits_equal(first, all_bits(dev, seed, 200))
        n_tests = dev.n_tests
    with open_case("n1000", model, alleles_only=True) as alone:
        assert alone.n_tests == n_allele < n_tests
        got = all_bits(alone, seed, 200)
    per = 2 if model == "genotype" else 1
    cut = {0: n_allele, 1: n_allele, 2: n_allele, 4: per * n_allele, 5: per * n_allele, 7: n_allele, 8: n_allele, 10: n_allele}
    # cnt, S1, S2, ybar, proj, g, rr, stat, flags, max_stat, count: the per-test arrays cut to the alleles; max_stat is a
    # maximum over MORE tests in the larger handle, so it is compared where the alleles hold the maximum
    for k, a in enumerate(first):
        if k == 9:
            continue
        b = a[:cut[k]] if k in cut else a
        assert b.tobytes() == got[k].tobytes(), k
    assert (got[9] <= first[9]).all() and (got[9] == first[9]).sum() >= 50


# 4 end to end -------------------------------------------------------------------------------------------------------------
def assert_results_close(got, want, tol):
    assert got.name == want.name and np.array_equal(got.flags, want.flags) and np.array_equal(got.counts, want.counts)
    assert (got.n_samp, got.n_excluded, got.n_perm, got.seed) == (want.n_samp, want.n_excluded, want.n_perm, want.seed)
    assert got.covariates == want.covariates and np.array_equal(got.df, want.df, equal_nan=True)
    for key in ("avg", "est", "se", "lower", "upper", "pval", "stat", "stat_p", "rss") + (("perm_p", "perm_p_adj", "max_stat") if want.n_perm else ()):
        assert np.array_equal(np.isnan(getattr(got, key)), np.isnan(getattr(want, key))), key
    ok = want.flags == 0
    assert ok.sum() >= 10
    scale = np.fmax(np.abs(want.est), want.se)
    # g moves by tol sqrt(xx rr) at most, est = g / sxx with it; in units of se = sqrt(rss / (df sxx)) that is tol sqrt(df xx / sxx)
    # -- bounded with xx / sxx <= 1e3 for these columns and rss >= rr / 2
    lim = tol * np.sqrt(2e3 * np.nanmax(want.df))
    assert np.nanmax(np.abs(got.est - want.est) / scale) <= lim and np.nanmax(np.abs(got.se / want.se - 1)) <= lim
    assert np.nanmax(np.abs(got.lower - want.lower) / scale) <= 3 * lim and np.nanmax(np.abs(got.upper - want.upper) / scale) <= 3 * lim
    assert np.nanmax(np.abs(got.stat - want.stat) / np.fmax(want.stat, 1)) <= tol
    assert np.nanmax(np.abs(got.rss / want.rss - 1)) <= lim and np.nanmax(np.abs(got.avg / want.avg - 1)) <= tol
    t = np.abs(want.est / want.se)
    fin = np.isfinite(t)
    assert (np.abs(np.log(got.pval[fin] / want.pval[fin])) <= 4 * lim * (1 + t[fin]) ** 2 + 1e-12).all()
    fin = np.isfinite(want.stat_p)
    assert (np.abs(np.log(got.stat_p[fin] / want.stat_p[fin])) <= 4 * lim * (1 + want.stat[fin]) + 1e-12).all()
    p = want.ttest_p if want.ttest_p is not None else want.anova_p
    gp = got.ttest_p if want.ttest_p is not None else got.anova_p
    fin = np.isfinite(p)
    assert np.array_equal(np.isnan(gp), np.isnan(p)) and (np.abs(np.log(gp[fin] / p[fin])) <= 1e-9).all()
    if want.n_perm:
        assert np.allclose(got.max_stat, want.max_stat, rtol=tol, atol=0)
        assert np.array_equal(got.perm_p, want.perm_p, equal_nan=True) and np.array_equal(got.perm_p_adj, want.perm_p_adj, equal_nan=True)
    else:
        assert got.perm_p is None and got.max_stat is None


def test_hla_assoc_quant_end_to_end_and_conditioned():
    hla, y, groups, covar = Q.hla_of("n1000")
    tol = Q.tolerance("n1000", "dominant")
    seed = Q.seed_of("n1000", "dominant")
    want = hb.hlaAssocQuant(hla, y, covar, groups=groups, n_perm=65, seed=seed, _backend=Q.Backend)
    got = hb.hlaAssocQuant(hla, y, covar, groups=groups, n_perm=65, seed=seed)
    assert_results_close(got, want, tol)
    assert got.flags[-1] == 2 and got.name[-1] == "pos:beyond"                  # a level the device does not know
    top = got.name[int(np.nanargmax(got.stat))]
    assert top == want.name[int(np.nanargmax(want.stat))]
    cwant = hb.hlaAssocQuant(hla, y, covar, groups=groups, condition=[top], n_perm=65, seed=seed, _backend=Q.Backend)
    cgot = hb.hlaAssocQuant(hla, y, covar, groups=groups, condition=[top], n_perm=65, seed=seed)
    assert cgot.flags[got.name.index(top)] & 2 and cgot.covariates[-1] == f"h[{top}]"
    assert_results_close(cgot, cwant, tol)
    # the genotype model, no permutations, collinear covariates
    hla, y, groups, covar = Q.hla_of("n257")
    assert_results_close(hb.hlaAssocQuant(hla, y, covar, model="genotype"), hb.hlaAssocQuant(hla, y, covar, model="genotype", _backend=Q.Backend),
                         Q.tolerance("n257", "genotype"))
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocQuant(hla, y, np.column_stack([covar[:, 0], 1 - 3 * covar[:, 0]]))


# 5 errors -----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0, 1, 1], np.int32)
    b = np.array([0, 0, 1, 1, 0, 1, 0, 1], np.int32)
    y = np.array([1.0, 2.5, -1.0, 4.0, 0.5, 3.0, 2.0, 7.0])
    cov = (np.arange(13 * 8, dtype=np.float64).reshape(13, 8) ** 2) % 7
    err = L.hibag_hip_last_error
    with assocquant._DeviceQuant(a, b, np.zeros(8, np.int32), 2, None, 0) as dev, \
            assocquant._DeviceQuant(a, b, np.zeros(8, np.int32), 2, None, 3) as gen:
        new = L.hibag_hip_assoc_quant_new
        assert not new(None, p(y), None, 0) and b"hibag_hip_assoc_quant_new" in err()
        assert not new(dev._h, None, None, 0)
        assert not new(dev._h, p(y), None, 1) and not new(dev._h, p(y), p(cov), -1)
        assert not new(dev._h, p(y), p(cov), 13) and b"13 covariates" in err()
        for v in (np.nan, np.inf):
            bad = y.copy()
            bad[6] = v
            assert not new(dev._h, p(bad), None, 0) and b"not finite" in err()
            badc = cov.copy()
            badc[1, 2] = v
            assert not new(dev._h, p(y), p(badc), 2) and b"not finite" in err()
        assert not new(dev._h, p(y), p(cov), 6) and b"degrees of freedom" in err()            # 8 - 1 - 6 - 1 = 0
        assert not new(gen._h, p(y), p(cov), 5) and b"degrees of freedom" in err()            # 8 - 1 - 5 - 2 = 0
        twice = np.stack([cov[0], 2 * cov[0] - 1])
        assert not new(dev._h, p(y), p(twice), 2) and b"collinear" in err()
        q5 = new(dev._h, p(y), p(cov), 5)
        assert q5
        L.hibag_hip_assoc_quant_free(q5)
        L.hibag_hip_assoc_quant_free(None)
        dev.quant(y, cov[:2])
        T = dev.n_tests
        cnt, S1, S2, ybar = np.empty((T, 3), np.int64), np.empty((T, 3)), np.empty((T, 3)), np.empty(1)
        outs = [p(cnt), p(S1), p(S2), p(ybar)]
        assert L.hibag_hip_assoc_quant_classes(dev._q, *outs) == 0 and abs(ybar[0] - y.mean()) < 1e-14
        for k in range(4):
            o = list(outs)
            o[k] = None
            assert L.hibag_hip_assoc_quant_classes(dev._q, *o) == -1
        assert L.hibag_hip_assoc_quant_classes(None, *outs) == -1
        proj, g, rr, stat, fl = np.empty((T, 3)), np.empty(T), np.empty(1), np.empty(T), np.empty(T, np.int32)
        outs = [p(proj), p(g), p(rr), p(stat), p(fl)]
        assert L.hibag_hip_assoc_quant_observed(dev._q, *outs) == 0
        for k in range(5):
            o = list(outs)
            o[k] = None
            assert L.hibag_hip_assoc_quant_observed(dev._q, *o) == -1
        assert L.hibag_hip_assoc_quant_observed(None, *outs) == -1
        ms, cp = np.empty(4), np.empty(T, np.int64)
        perm = L.hibag_hip_assoc_quant_permute
        assert perm(dev._q, 1, 1, 4, p(ms), p(cp)) == 0 and np.isfinite(ms).all()
        assert perm(dev._q, 1, 1, 0, None, p(cp)) == 0 and (cp == 0).all()
        assert perm(dev._q, 1, 0, 4, p(ms), p(cp)) == -1 and b"numbered from 1" in err()
        assert perm(dev._q, 1, (1 << 64) - 2, 4, p(ms), p(cp)) == -1
        assert perm(dev._q, 1, 1, -1, p(ms), p(cp)) == -1 and perm(dev._q, 1, 1, 4, None, p(cp)) == -1
        assert perm(dev._q, 1, 1, 4, p(ms), None) == -1 and perm(None, 1, 1, 4, p(ms), p(cp)) == -1
        rows = np.empty((2, 8), np.int32)
        pr = L.hibag_hip_assoc_quant_perm_rows
        assert pr(dev._q, 1, 1, 2, p(rows)) == 0 and (np.sort(rows, axis=1) == np.arange(8)).all()
        assert pr(dev._q, 1, 0, 2, p(rows)) == -1 and pr(dev._q, 1, 1, -1, p(rows)) == -1 and pr(dev._q, 1, 1, 2, None) == -1
        assert pr(None, 1, 1, 2, p(rows)) == -1 and pr(dev._q, 1, (1 << 64) - 1, 2, p(rows)) == -1
        import ctypes as C
        t = C.c_double(-1.0)
        assert L.hibag_hip_assoc_quant_gram_ms(dev._q, C.byref(t)) == 0 and t.value >= 0.0
        assert L.hibag_hip_assoc_quant_gram_ms(None, C.byref(t)) == -1 and L.hibag_hip_assoc_quant_gram_ms(dev._q, None) == -1
