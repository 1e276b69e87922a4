"""hlaAssocScore on the GPU: the hibag_hip_assoc_score_* entries against the restatement (tests/assocscore_reference.py:
DESIGN.md section 28 in numpy) -- the signs byte for byte; flags, degrees of freedom, kept-column masks and replicate counts
equal as integers; the projections, set Grams, scores, statistics and per-replicate maxima within a tolerance computed from
the restatement alone (100 x its float64-versus-longdouble difference over the case, at least 1e-12; each quantity in units
of its own scale, ``assocscore_reference.differences``) --, at cohort sizes around the 128-sample padding and the 16-row
tiles, for the four models, sets of 1 .. 30 rows and 1 .. 200 replicates; results bit-equal across panel sizes, split
calls, handles with more tests, repeated calls and other entries' calls in between; hlaAssocScore end to end; invalid
arguments rejected.

The integer comparisons of the counts rest on the safety condition that tests/test_assocscore_host.py asserts for every case
here: no resampled statistic within 1e-6 relative of its observed one, no replicate's smallest p-value within 1e-6 relative
of an observed one.  The measured device differences are in DESIGN.md section 28, "Checks"."""
import numpy as np
import pytest

import hibag_amd as hb
import assocscore_reference as SR
from hibag_amd import _lib, assoc, assocscore

pytestmark = pytest.mark.gpu

MODELS = SR.MODELS


def open_case(case, model, alleles_only=False):
    A, covar, _, (a1, a2, y, n_allele, g) = SR.analysis(case, model)
    dev = assocscore._DeviceScore(a1, a2, y, n_allele, None if alleles_only else g, MODELS.index(model))
    assert dev.n_kept == A.n
    dev.score(covar, None, 25, 1e-8)
    return dev


# 1 the generator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["n5", "n257", "n1000"])
def test_signs_byte_for_byte(case):
    with open_case(case, "dominant") as dev:
        n = dev.n_kept
        for rows, seed, p0 in ((1, 0, 1), (2, 0xFFFFFFFFFFFFFFFF, (1 << 64) - 3), (127, 0x0123456789ABCDEF, (1 << 40) + 7),
                               (128, 1 << 32, (1 << 32) - 64), (129, 0x9E3779B97F4A7C15, 1 << 63), (300, 12345, 1), (3, 77, 127),
                               (2, 77, 128), (2, 77, 129)):
            got = dev.score_signs(seed, p0, rows)
            want = SR.signs(seed, p0, rows, n)
            assert got.dtype == np.int8 and got.shape == (rows, n)
            assert got.tobytes() == want.tobytes(), (case, rows, seed, p0)
        assert dev.score_signs(3, 5, 0).shape == (0, n)


def test_signs_across_panels(monkeypatch):
    """40 rows in panels of 16, 16 and 8: each panel reaches the host before the next overwrites the device's buffer."""
    monkeypatch.setenv("HIBAG_SCORE_PANEL_PERMS", "16")
    with open_case("n40", "dominant") as dev:
        assert dev.score_signs(9, 120, 40).tobytes() == SR.signs(9, 120, 40, dev.n_kept).tobytes()


# 2 values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(SR.CASES))
def test_numbers_equal_the_restatement(case, model):
    Z = SR.reference(case, model)
    tol = SR.tolerance(case, model)
    want = SR.numbers(Z)
    with open_case(case, model) as dev:
        assert dev.n_rows == len(Z.F)
        coef, se, deviance, it, fl = dev.score_base()
        assert fl == Z.base["flags"] and it == Z.base["iterations"]
        proj, S, kept = dev.score_sets(Z.sets)
        g, stat, df, flags = dev.score_observed()
        assert kept.dtype == np.int32 and np.array_equal(kept, Z.kept), (kept, Z.kept)
        assert np.array_equal(df, Z.df) and np.array_equal(flags, Z.flags), (df, Z.df, flags, Z.flags)
        assert np.array_equal(np.isnan(stat), np.isnan(np.asarray(Z.stat, np.float64))) and np.isnan(stat[Z.df == 0]).all()
        for n_perm in SR.PERM_COUNTS[case]:
            max_stat, count = dev.score_resample(Z.seed, 1, n_perm)
            assert max_stat.shape == (n_perm, len(Z.dfs))
            assert np.array_equal(np.isnan(max_stat), np.isnan(Z.max_stat[:n_perm]))
            got = dict(proj=proj, S=S, g=g, stat=stat, max_stat=max_stat)
            d = SR.differences(got, dict(want, max_stat=Z.max_stat[:n_perm]))
            print(f"{case} {model} {n_perm} replicates: tol {tol:.3g}, device differences " +
                  " ".join(f"{k} {v:.3g}" for k, v in d.items()) + f" ({max(d.values()) / tol:.3g} of tol)")
            assert max(d.values()) <= tol, d
            with np.errstate(invalid="ignore"):
                want_count = (Z.perm_T[:, :n_perm] >= Z.stat[:, None]).sum(axis=1)
            assert count.dtype == np.int64 and np.array_equal(count, want_count), (count, want_count)


# 3 reproducibility --------------------------------------------------------------------------------------------------------
def all_bits(dev, sets, seed, n_perm):
    proj, S, kept = dev.score_sets(sets)
    out = [proj, kept] + list(S) + list(dev.score_observed()) + list(dev.score_resample(seed, 1, n_perm))
    return [np.asarray(a) for a in out]


def bits_equal(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["dominant", "genotype"])
def test_results_are_bit_equal(model, monkeypatch):
    """Panels of 16 and 48 against the default; two calls of 100 against one of 200; the same call twice; the alleles alone
    against the alleles with the partition's tests beside them; before and after a permutation call, a regression call and a
    quantitative-trait permutation call on the same handle."""
    seed = 0xC0FFEE1234567890
    A = SR.analysis("n1000", model)[0]
    n_allele = SR.CASES["n1000"][1]
    per = 2 if model == "genotype" else 1
    sets = SR.single_sets(model, A.rsum, A.n)[:n_allele] + [list(range(1, 31)), list(range(2, 19))]     # (rows of the alleles alone)
    assert max(max(s) for s in sets if s) < per * n_allele
    with open_case("n1000", model) as dev:
        first = all_bits(dev, sets, seed, 200)
        assert bits_equal(first, all_bits(dev, sets, seed, 200))
        monkeypatch.setenv("HIBAG_SCORE_PANEL_PERMS", "16")
        assert bits_equal(first, all_bits(dev, sets, seed, 200))
        monkeypatch.setenv("HIBAG_SCORE_PANEL_PERMS", "48")                       # (a last panel of 8: half a tile)
        assert bits_equal(first, all_bits(dev, sets, seed, 200))
        monkeypatch.delenv("HIBAG_SCORE_PANEL_PERMS")
        m1, c1 = dev.score_resample(seed, 1, 100)
        m2, c2 = dev.score_resample(seed, 101, 100)
        assert np.concatenate([m1, m2]).tobytes() == first[-2].tobytes() and np.array_equal(c1 + c2, first[-1])
        dev.permute(11, 1, 300)
        dev.glm(None, None, 25, 1e-8)
        L, p = _lib.lib(), assoc._ptr
        trait = np.random.default_rng(5).standard_normal(dev.n_kept)
        q = L.hibag_hip_assoc_quant_new(dev._h, p(trait), None, 0)                # a quantitative trait on the same handle
        assert q
        ms, cp = np.empty(40), np.empty(dev.n_tests, np.int64)
        assert L.hibag_hip_assoc_quant_permute(q, 3, 1, 40, p(ms), p(cp)) == 0
        L.hibag_hip_assoc_quant_free(q)
        assert bits_equal(first, all_bits(dev, sets, seed, 200))
        n_rows = dev.n_rows
    with open_case("n1000", model, alleles_only=True) as alone:
        assert alone.n_rows == per * n_allele < n_rows
        got = all_bits(alone, sets, seed, 200)
    # proj and g hold every row of the handle: cut to the alleles' rows; everything else is per set
    first[0], first[2 + len(sets)] = first[0][:per * n_allele], first[2 + len(sets)][:per * n_allele]
    assert bits_equal(first, got)


# 4 end to end -------------------------------------------------------------------------------------------------------------
def assert_results_close(got, want, tol):
    assert got.name == want.name and np.array_equal(got.flags, want.flags) and np.array_equal(got.df, want.df)
    assert (got.n_samp, got.n_case, got.n_excluded, got.n_perm, got.seed) == (want.n_samp, want.n_case, want.n_excluded, want.n_perm, want.seed)
    assert got.base["name"] == want.base["name"] and got.base["flags"] == want.base["flags"]
    assert np.allclose(got.base["est"], want.base["est"], rtol=1e-9, atol=1e-12)
    for key in ("score_stat", "score_p") + (("perm_p", "perm_p_adj", "max_stat", "min_p") if want.n_perm else ()):
        assert np.array_equal(np.isnan(getattr(got, key)), np.isnan(getattr(want, key))), key
    ok = want.flags == 0
    assert ok.sum() >= 1
    assert np.nanmax(np.abs(got.score_stat - want.score_stat) / np.fmax(want.score_stat, 1)) <= tol
    fin = np.isfinite(want.score_p)
    # d log p / dT is at most 1/2 in the tail (and the tail's own relative error is a few ulp)
    assert (np.abs(np.log(got.score_p[fin] / want.score_p[fin])) <= tol * np.fmax(want.score_stat[fin], 1) + 1e-12).all()
    if want.n_perm:
        assert np.array_equal(got.max_stat_df, want.max_stat_df)
        assert np.allclose(got.max_stat, want.max_stat, rtol=tol, atol=tol, equal_nan=True)
        assert np.array_equal(got.perm_p, want.perm_p, equal_nan=True) and np.array_equal(got.perm_p_adj, want.perm_p_adj, equal_nan=True)
    else:
        assert got.perm_p is None and got.max_stat is None


def test_hla_assoc_score_end_to_end_and_conditioned():
    hla, y, groups, covar = SR.hla_of("n1000")
    tol = SR.tolerance("n1000", "dominant")
    seed = SR.seed_of("n1000", "dominant")
    want = hb.hlaAssocScore(hla, y, covar, groups=groups, n_perm=65, seed=seed, _backend=SR.Backend)
    got = hb.hlaAssocScore(hla, y, covar, groups=groups, n_perm=65, seed=seed)
    assert_results_close(got, want, tol)
    assert got.flags[-1] == 2 and got.name[-1] == "pos:beyond"                  # a level the device does not know
    top = got.name[int(np.nanargmax(got.score_stat))]
    assert top == want.name[int(np.nanargmax(want.score_stat))]
    cwant = hb.hlaAssocScore(hla, y, covar, groups=groups, condition=[top], n_perm=65, seed=seed, _backend=SR.Backend)
    cgot = hb.hlaAssocScore(hla, y, covar, groups=groups, condition=[top], n_perm=65, seed=seed)
    assert cgot.flags[got.name.index(top)] & 2 and cgot.base["name"][-1] == f"h[{top}]"
    assert_results_close(cgot, cwant, tol)
    # the omnibus form, the genotype model without replicates, prior weights, collinear covariates
    assert_results_close(hb.hlaAssocScore(hla, y, covar, "additive", groups=groups, omnibus=True, n_perm=65, seed=seed),
                         hb.hlaAssocScore(hla, y, covar, "additive", groups=groups, omnibus=True, n_perm=65, seed=seed, _backend=SR.Backend), tol)
    hla, y, groups, covar = SR.hla_of("n257")
    tolg = SR.tolerance("n257", "genotype")
    assert_results_close(hb.hlaAssocScore(hla, y, covar, model="genotype"), hb.hlaAssocScore(hla, y, covar, model="genotype", _backend=SR.Backend), tolg)
    assert_results_close(hb.hlaAssocScore(hla, y, covar, use_prob=True), hb.hlaAssocScore(hla, y, covar, use_prob=True, _backend=SR.Backend), tolg)
    with pytest.raises(ValueError, match="collinear"):
        hb.hlaAssocScore(hla, y, np.column_stack([covar[:, 0], 1 - 3 * covar[:, 0]]))


# 5 errors -----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p = assoc._ptr
    a = np.array([0, 1, 0, 1, 0, 0, 1, 1] * 8, np.int32)
    b = np.array([0, 0, 1, 1, 0, 1, 0, 1] * 8, np.int32)
    y = (np.arange(64) * 7 % 5 < 2).astype(np.int32)
    n = 64
    cov = ((np.arange(13 * n, dtype=np.float64).reshape(13, n) ** 2) % 7) / 7
    err = L.hibag_hip_last_error
    i32 = lambda v: np.array(v, np.int32)      # noqa: E731
    with assocscore._DeviceScore(a, b, y, 32, None, 0) as dev:
        new = L.hibag_hip_assoc_score_new
        assert not new(None, None, 0, None, 25, 1e-8) and b"hibag_hip_assoc_score_new" in err()
        assert not new(dev._h, None, 1, None, 25, 1e-8) and not new(dev._h, p(cov), -1, None, 25, 1e-8)
        assert not new(dev._h, p(cov), 13, None, 25, 1e-8) and b"13 covariates" in err()
        assert not new(dev._h, None, 0, None, 0, 1e-8) and not new(dev._h, None, 0, None, 25, 0.0)
        for v in (np.nan, np.inf):
            badc = cov.copy()
            badc[1, 2] = v
            assert not new(dev._h, p(badc), 2, None, 25, 1e-8) and b"not finite" in err()
        wt = np.ones(n)
        wt[3] = -1.0
        assert not new(dev._h, None, 0, p(wt), 25, 1e-8) and b"weight" in err()
        twice = np.stack([cov[0], 2 * cov[0] - 1])
        assert not new(dev._h, p(twice), 2, None, 25, 1e-8) and b"collinear" in err()
        s2 = new(dev._h, p(cov), 2, None, 25, 1e-8)
        assert s2
        L.hibag_hip_assoc_score_free(s2)
        L.hibag_hip_assoc_score_free(None)
        dev.score(cov[:2], None, 25, 1e-8)
        R = dev.n_rows
        assert R == 32
        proj, S, kept = np.empty((R, 3)), np.empty(31 * 31 + 4), np.empty(4, np.int32)
        g, stat, df, fl = np.empty(R), np.empty(2), np.empty(2, np.int32), np.empty(2, np.int32)
        ms, cp = np.empty(8), np.empty(2, np.int64)
        sets, obs, res = L.hibag_hip_assoc_score_sets, L.hibag_hip_assoc_score_observed, L.hibag_hip_assoc_score_resample
        assert obs(dev._s, p(g), p(stat), p(df), p(fl)) == -1 and b"no sets" in err()
        assert res(dev._s, 1, 1, 4, p(ms), p(cp)) == -1 and L.hibag_hip_assoc_score_n_df(dev._s) == -1
        start, rows = i32([0, 1, 2]), i32([0, 1])
        assert sets(dev._s, p(i32([0, 31])), p(i32(list(range(31)))), 1, p(proj), p(S), p(kept)) == -1 and b"at most 30" in err()
        assert sets(dev._s, p(i32([0, 30])), p(i32(list(range(30)))), 1, p(proj), p(S), p(kept)) == 0
        assert sets(dev._s, p(i32([1, 2])), p(rows), 1, p(proj), p(S), p(kept)) == -1
        assert sets(dev._s, p(i32([0, 2, 1])), p(rows), 2, p(proj), p(S), p(kept)) == -1 and b"monotone" in err()
        assert sets(dev._s, p(i32([0, 2])), p(i32([0, 0])), 1, p(proj), p(S), p(kept)) == -1 and b"twice" in err()
        assert sets(dev._s, p(i32([0, 1])), p(i32([R])), 1, p(proj), p(S), p(kept)) == -1 and b"outside" in err()
        assert sets(dev._s, p(i32([0, 1])), p(i32([-1])), 1, p(proj), p(S), p(kept)) == -1
        assert sets(dev._s, p(start), None, 2, p(proj), p(S), p(kept)) == -1 and sets(dev._s, None, p(rows), 2, p(proj), p(S), p(kept)) == -1
        assert sets(dev._s, p(start), p(rows), -1, p(proj), p(S), p(kept)) == -1
        assert sets(None, p(start), p(rows), 2, p(proj), p(S), p(kept)) == -1
        for k in range(3):
            o = [p(proj), p(S), p(kept)]
            o[k] = None
            assert sets(dev._s, p(start), p(rows), 2, *o) == -1
        assert sets(dev._s, p(start), p(rows), 2, p(proj), p(S), p(kept)) == 0 and (kept[:2] == 1).all()
        outs = [p(g), p(stat), p(df), p(fl)]
        assert obs(dev._s, *outs) == 0 and (df == 1).all() and (fl == 0).all() and L.hibag_hip_assoc_score_n_df(dev._s) == 1
        for k in range(4):
            o = list(outs)
            o[k] = None
            assert obs(dev._s, *o) == -1
        assert obs(None, *outs) == -1
        assert res(dev._s, 1, 1, 4, p(ms), p(cp)) == 0 and np.isfinite(ms[:4]).all()
        assert res(dev._s, 1, 1, 0, None, p(cp)) == 0 and (cp == 0).all()
        assert res(dev._s, 1, 0, 4, p(ms), p(cp)) == -1 and b"numbered from 1" in err()
        assert res(dev._s, 1, (1 << 64) - 2, 4, p(ms), p(cp)) == -1
        assert res(dev._s, 1, 1, -1, p(ms), p(cp)) == -1 and res(dev._s, 1, 1, 4, None, p(cp)) == -1
        assert res(dev._s, 1, 1, 4, p(ms), None) == -1 and res(None, 1, 1, 4, p(ms), p(cp)) == -1
        sg = np.empty((2, n), np.int8)
        sn = L.hibag_hip_assoc_score_signs
        assert sn(dev._s, 1, 1, 2, p(sg)) == 0 and (np.abs(sg) == 1).all()
        assert sn(dev._s, 1, 0, 2, p(sg)) == -1 and sn(dev._s, 1, 1, -1, p(sg)) == -1 and sn(dev._s, 1, 1, 2, None) == -1
        assert sn(None, 1, 1, 2, p(sg)) == -1 and sn(dev._s, 1, (1 << 64) - 1, 2, p(sg)) == -1
        t = np.full(3, -1.0)
        assert L.hibag_hip_assoc_score_ms(dev._s, p(t)) == 0 and (t >= 0).all()
        assert L.hibag_hip_assoc_score_ms(None, p(t)) == -1 and L.hibag_hip_assoc_score_ms(dev._s, None) == -1
        base = [np.empty(16), np.empty(16), np.empty(1), np.empty(1, np.int32), np.empty(1, np.int32)]
        assert L.hibag_hip_assoc_score_base(dev._s, *[p(x) for x in base]) == 0 and base[4][0] == 0 and np.isfinite(base[0][[0, 3, 4]]).all()
        assert L.hibag_hip_assoc_score_base(None, *[p(x) for x in base]) == -1
        assert L.hibag_hip_assoc_score_base(dev._s, None, *[p(x) for x in base[1:]]) == -1
        # an empty list of sets is allowed: nothing to test, no degrees of freedom
        assert sets(dev._s, p(i32([0])), None, 0, p(proj), None, None) == 0 and L.hibag_hip_assoc_score_n_df(dev._s) == 0
        assert res(dev._s, 1, 1, 4, p(ms), p(cp)) == 0
