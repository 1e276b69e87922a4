"""hlaAssocHaplo on the GPU.

1. ``hibag_hip_haplo_dosage`` against the restatement (tests/assochaplo_reference.py) bit for bit: every dosage is a
   sequential sum of posteriors in a defined order, so there is no tolerance.
2. ``hibag_hip_assoc_rscore_sets`` and the observed / resampled runs over real-valued rows against the restatement:
   flags, degrees of freedom, kept masks and replicate counts equal as integers; proj, S, g, stat and max_stat within a
   tolerance computed from the restatement alone (100 x its float64-versus-longdouble difference over the case, at least
   1e-12, in section 28's scales with sum x^2 in place of the integer sums); device against device bit for bit across panel
   sizes, split calls, a subset of the rows, repeated calls and int8 installs around a real one; rows of 0 / 1 / 2 against
   the int8 path.
3. ``hlaAssocHaplo`` end to end against the same call on the restatement back end.

The integer comparisons of the counts rest on the safety conditions that tests/test_assochaplo_host.py asserts for every case
here.  The measured device differences are in DESIGN.md section 30, "Checks"."""
import numpy as np
import pytest

import hibag_amd as hb
import assochaplo_reference as HR
import assocscore_reference as SR
import haplo_reference as R
from hibag_amd import NA_INTEGER, _lib, assoc, assocscore, haplo
from hibag_amd.topk import HlaTopCalls

pytestmark = pytest.mark.gpu

NA = NA_INTEGER


# 1 the dosage -------------------------------------------------------------------------------------------------------------
def device_dosage(h1, h2, prob, hap=None, max_states=4096, min_prob=0.01, maxit=200, tol=1e-8, refit=False):
    """The device's dosages of the haplotypes `hap` (all, in ascending-key order, by default) for candidates [L][n][k], trimmed
    as hlaHaplotypes trims them."""
    t1, t2, tp, _ = haplo.trim_candidates(h1, h2, prob, min_prob, max_states)
    with haplo._DeviceHaplo(t1, t2, tp, max_states) as dev:
        if refit:
            dev.fit(2, 0.0)
        fit = dev.fit(maxit, tol)
        return fit, dev.dosage(np.arange(dev.n_hap) if hap is None else hap)


def assert_dosage_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} dosages differ, the first at {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def hand_cohort():
    h1 = np.array([[[0, 0], [0, NA], [0, 1]], [[2, 2], [2, NA], [3, NA]]], np.int32)
    h2 = np.array([[[1, 0], [0, NA], [1, 1]], [[3, 2], [2, NA], [3, NA]]], np.int32)
    prob = np.array([[[.7, .3], [1., 0.], [.9, .1]], [[.6, .4], [1., 0.], [1., 0.]]])
    return h1, h2, prob


def test_dosage_of_three_samples_by_hand():
    r = HR.dosages(*hand_cohort())
    fit, D = device_dosage(*hand_cohort())
    assert np.array_equal(fit["keys"], r["keys"])
    assert_dosage_bits(D, r["D"], "by hand")
    assert D[0, 1] == 2.0 and D[1, 1] == 0.0 and D[0, 2] == 0.0 and D[3, 1] == 0.0      # one homozygous state; absent: exactly 0


@pytest.fixture(scope="module")
def ld_case():
    """The 130 x 3 x 3 cohort of tests/test_hip_haplo.py's kind: NA ranks, a sample left out, an all-homozygous sample."""
    _, h1, h2, prob = R.ld_cohort(130, 3, 3, 8, 12, seed=11)
    h1[0, 3::7, 2] = NA; h2[0, 3::7, 2] = NA; prob[0, 3::7, 2] = 0.0
    h1[1, 4::9, 1] = NA; h2[1, 4::9, 1] = NA; prob[1, 4::9, 1] = 0.0
    h1[1, 5, :] = NA; h2[1, 5, :] = NA; prob[1, 5, :] = 0.0
    for l in range(3):
        h1[l, 7, :], h2[l, 7, :], prob[l, 7, :] = [l + 1, NA, NA], [l + 1, NA, NA], [1.0, 0.0, 0.0]
    return (h1, h2, prob), HR.dosages(h1, h2, prob)


def test_dosage_on_the_ld_cohort(ld_case):
    arrays, r = ld_case
    H = len(r["keys"])
    fit, D = device_dosage(*arrays)
    assert fit["freq"].tobytes() == r["freq"].tobytes()
    assert_dosage_bits(D, r["D"], "LD cohort, m = H")
    assert np.isnan(D[:, 5]).all() and not np.isnan(np.delete(D, 5, axis=1)).any()
    assert sorted(D[:, 7][D[:, 7] != 0].tolist()) == [2.0]                                 # the all-homozygous sample
    assert (D[:, r["used"]] == 0.0).any()
    # m = 1, m = 17 (any order, a haplotype twice), and after a second fit on the same handle
    for hap in ([H - 1], [int(np.argmax(r["freq"]))], list(range(16, -1, -1)), [3, 3, 0]):
        _, d = device_dosage(*arrays, hap=np.array(hap, np.int32), refit=True)
        assert_dosage_bits(d, r["D"][hap], f"hap = {hap}")


def test_dosage_of_lists_longer_than_a_workgroup():
    """Lists of more than 256, 512 and 768 entries: a thread of k_haplo_dosage looks at several positions of one list, and a
    segment's head and its tail fall to different threads."""
    _, h1, h2, prob = R.ld_cohort(300, 2, 3, 3, 5, seed=7)
    r = HR.dosages(h1, h2, prob, maxit=6)
    lengths = sorted(len(v) for v in r["lists"])
    assert lengths[-1] > 768 and any(256 < v <= 512 for v in lengths), lengths[-6:]
    fit, D = device_dosage(h1, h2, prob, maxit=6)
    assert fit["freq"].tobytes() == r["freq"].tobytes()
    assert_dosage_bits(D, r["D"], "long lists")


SEGMENTS = ((1, 1, 18, 18), (2, 1, 18, 18), (9, 7, 18, 18), (8, 8, 18, 18), (5, 13, 18, 18), (3, 43, 6, 54))


def segment_cohort():
    """L = 2.  Six samples of 648 states each -- n0 and n1 heterozygous candidates at the two loci, 2 n0 2 n1 / 2 = 648 -- in
    which the haplotype (a, b) of the sample (alleles of its own) is in c0 candidates at locus 0 and c1 at locus 1, so that
    its segment has c0 c1 = 1, 2, 63, 64, 65 and 129 entries; the candidates' weights are random, so the posteriors are
    unequal.  Then the 648-state sample of tests/test_hip_haplo.py's seams, and two samples that share sample 3's
    haplotype."""
    rng = np.random.default_rng(12)
    k = 54
    rows = []

    def weights(n):
        return np.sort(rng.dirichlet(np.full(n, 3.0)))[::-1]

    def locus(target, c, n, base):
        """n heterozygous pairs, c of them with `target`; the other alleles from `base` up, each once."""
        pairs = [(target, base + j) for j in range(c)] + [(base + c + 2 * j, base + c + 2 * j + 1) for j in range(n - c)]
        order = rng.permutation(n)
        return [(min(pairs[j]), max(pairs[j]), p) for j, p in zip(order, weights(n))]

    for i, (c0, c1, n0, n1) in enumerate(SEGMENTS):
        rows.append([locus(150 * i, c0, n0, 150 * i + 1), locus(150 * i, c1, n1, 150 * i + 1)])
    rows.append([[(0, 1, .5), (900, 901, .3), (902, 903, .2)], [(0, 1, .6), (900, 901, .4)]])       # shares (0, 0)-side alleles
    a = 150 * 3
    rows.append([[(a, a, 1.0)], [(a, a, 1.0)]])                          # sample 3's haplotype, homozygous: exactly 2.0
    rows.append([[(a, a + 1, 1.0)], [(a, 999, .7), (a, a, .3)]])
    n = len(rows)
    h1, h2, prob = np.full((2, n, k), NA, np.int32), np.full((2, n, k), NA, np.int32), np.zeros((2, n, k))
    for s, row in enumerate(rows):
        for l, c in enumerate(row):
            for j, (x, y, p) in enumerate(c):
                h1[l, s, j], h2[l, s, j], prob[l, s, j] = x, y, p
    return h1, h2, prob


def test_dosage_segments_of_1_2_63_64_65_and_129_entries():
    h1, h2, prob = segment_cohort()
    kw = dict(min_prob=0.0, maxit=4)
    r = HR.dosages(h1, h2, prob, **kw)
    assert r["n_states"][:6].tolist() == [648] * 6
    keys = r["keys"].tolist()
    for i, (c0, c1, _, _) in enumerate(SEGMENTS):
        h = keys.index(150 * i + ((150 * i) << 10))
        seg = [e for e in r["lists"][h] if r["sample_of"][e // 2] == i]
        assert len(seg) == c0 * c1, (i, len(seg))
        assert len({float(r["q"][e // 2]) for e in seg}) == len(seg)                        # unequal posteriors
    fit, D = device_dosage(h1, h2, prob, **kw)
    assert np.array_equal(fit["keys"], r["keys"]) and fit["freq"].tobytes() == r["freq"].tobytes()
    assert_dosage_bits(D, r["D"], "segments")
    h3 = keys.index(450 + (450 << 10))
    assert D[h3, 7] == 2.0 and 0 < D[h3, 3] < 2 and D[h3, 8] > 0 and D[h3, 0] == 0.0
    # the 648-state sample of the seams cohort (L = 4)
    cand = [[(40, 41), (40, 42), (41, 43)], [(1, 2), (2, 3), (3, 4)], [(1, 2), (2, 3), (3, 4)], [(0, 1), (1, 2), (2, 3)]]
    g1, g2, gp = np.full((4, 2, 3), NA, np.int32), np.full((4, 2, 3), NA, np.int32), np.zeros((4, 2, 3))
    rng = np.random.default_rng(5)
    for l, c in enumerate(cand):
        w = np.sort(rng.dirichlet(np.full(3, 3.0)))[::-1]
        for j, (x, y) in enumerate(c):
            g1[l, 0, j], g2[l, 0, j], gp[l, 0, j] = x, y, w[j]
        g1[l, 1, 0], g2[l, 1, 0], gp[l, 1, 0] = c[0][0], c[0][0], 1.0
    r4 = HR.dosages(g1, g2, gp, min_prob=0.0)
    assert r4["n_states"].tolist() == [648, 1]
    _, D4 = device_dosage(g1, g2, gp, min_prob=0.0)
    assert_dosage_bits(D4, r4["D"], "648 states, four loci")


def test_hla_haplotypes_returns_dosages_in_result_order(ld_case):
    (h1, h2, prob), r = ld_case
    n = h1.shape[1]
    ids = [f"s{i}" for i in range(n)]
    calls = {f"L{l}": HlaTopCalls(f"L{l}", list(ids), 3, h1[l], h2[l], prob[l], np.ones(n), levels=[f"L{l}*{i:04d}" for i in range(12)])
             for l in range(3)}
    plain = hb.hlaHaplotypes(calls, verbose=False)
    assert plain.dosage is None and plain.dosage_index is None
    res = hb.hlaHaplotypes(calls, verbose=False, dosage_min_freq=0.01)
    assert res.freq.tobytes() == plain.freq.tobytes() and res.h1.tobytes() == plain.h1.tobytes()       # nothing else changes
    assert np.array_equal(res.dosage_index, np.flatnonzero(res.freq >= 0.01)) and 1 < len(res.dosage_index) < len(res.freq)
    at = {int(k): i for i, k in enumerate(r["keys"])}
    want = r["D"][[at[int(k)] for k in res.keys[res.dosage_index]]]
    assert_dosage_bits(res.dosage, want, "result order")
    everything = hb.hlaHaplotypes(calls, verbose=False, dosage_min_freq=0.0)
    assert everything.dosage.shape == (len(res.freq), n)
    assert np.nanmax(np.abs(everything.dosage.sum(axis=0) - 2.0)) < 1e-12


def test_dosage_rejects_invalid_arguments():
    L, p = _lib.lib(), assoc._ptr
    h1, h2, prob = hand_cohort()
    out, hap = np.empty((4, 3)), np.arange(4, dtype=np.int32)
    err = L.hibag_hip_last_error
    with haplo._DeviceHaplo(h1, h2, prob, 4096) as dev:
        assert L.hibag_hip_haplo_dosage(dev._h, p(hap), 4, p(out)) == -1 and b"hibag_hip_haplo_fit first" in err()      # before a fit
        dev.fit(5, 1e-8)
        assert L.hibag_hip_haplo_dosage(dev._h, p(hap), 4, p(out)) == 0
        assert L.hibag_hip_haplo_dosage(dev._h, p(hap), 0, p(out)) == -1 and L.hibag_hip_haplo_dosage(dev._h, p(hap), -3, p(out)) == -1
        for bad in (4, -1):
            assert L.hibag_hip_haplo_dosage(dev._h, p(np.array([0, bad], np.int32)), 2, p(out)) == -1 and b"0 .. 3" in err()
        assert L.hibag_hip_haplo_dosage(None, p(hap), 4, p(out)) == -1
        assert L.hibag_hip_haplo_dosage(dev._h, None, 4, p(out)) == -1 and L.hibag_hip_haplo_dosage(dev._h, p(hap), 4, None) == -1


# 2 real-valued rows -----------------------------------------------------------------------------------------------------
def open_case(case):
    A, covar, _, (a1, a2, y, n_allele, g) = SR.analysis(case, "additive")
    dev = assocscore._DeviceScore(a1, a2, y, n_allele, g, SR.MODELS.index("additive"))
    assert dev.n_kept == A.n
    dev.score(covar, None, 25, 1e-8)
    return dev


@pytest.mark.parametrize("case", list(HR.ROWS))
def test_real_rows_equal_the_restatement(case):
    Z = HR.reference(case)
    tol = HR.tolerance(case)
    want = SR.numbers(Z)
    X = HR.real_rows(case)
    with open_case(case) as dev:
        proj, S, kept = dev.score_real_sets(X, Z.sets)
        g, stat, df, flags = dev.score_observed()
        assert proj.shape == (len(X), Z.nb) and g.shape == (len(X),)
        assert kept.dtype == np.int32 and np.array_equal(kept, Z.kept), (kept, Z.kept)
        assert np.array_equal(df, Z.df) and np.array_equal(flags, Z.flags), (df, Z.df, flags, Z.flags)
        assert np.array_equal(np.isnan(stat), np.isnan(np.asarray(Z.stat, np.float64))) and np.isnan(stat[Z.df == 0]).all()
        for n_perm in SR.PERM_COUNTS[case]:
            max_stat, count = dev.score_resample(Z.seed, 1, n_perm)
            assert max_stat.shape == (n_perm, len(Z.dfs))
            assert np.array_equal(np.isnan(max_stat), np.isnan(Z.max_stat[:n_perm]))
            d = SR.differences(dict(proj=proj, S=S, g=g, stat=stat, max_stat=max_stat), dict(want, max_stat=Z.max_stat[:n_perm]))
            print(f"{case} {len(X)} rows {n_perm} replicates: tol {tol:.3g}, device differences " +
                  " ".join(f"{k} {v:.3g}" for k, v in d.items()) + f" ({max(d.values()) / tol:.3g} of tol)")
            assert max(d.values()) <= tol, d
            with np.errstate(invalid="ignore"):
                want_count = (Z.perm_T[:, :n_perm] >= Z.stat[:, None]).sum(axis=1)
            assert count.dtype == np.int64 and np.array_equal(count, want_count), (count, want_count)


def real_bits(dev, X, sets, seed, n_perm):
    proj, S, kept = dev.score_real_sets(X, sets)
    out = [proj, kept] + list(S) + list(dev.score_observed()) + list(dev.score_resample(seed, 1, n_perm))
    return [np.asarray(a) for a in out]


def int8_bits(dev, sets, seed, n_perm):
    proj, S, kept = dev.score_sets(sets)
    out = [proj, kept] + list(S) + list(dev.score_observed()) + list(dev.score_resample(seed, 1, n_perm))
    return [np.asarray(a) for a in out]


def bits_equal(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_real_rows_are_bit_equal_device_against_device(monkeypatch):
    """Panels of 16 and 48 against the default; two calls of 100 against one of 200; the same call twice; a subset of the rows
    alone against all the rows; the int8 sets before and after a real install on the same handle."""
    seed = 0xC0FFEE1234567890
    case = "n1000"
    X = HR.real_rows(case)
    m = len(X)
    sets = HR.real_sets(m)
    A = SR.analysis(case, "additive")[0]
    isets = SR.single_sets("additive", A.rsum, A.n)[:20] + [list(range(1, 31))]
    with open_case(case) as dev:
        before = int8_bits(dev, isets, seed, 200)
        first = real_bits(dev, X, sets, seed, 200)
        assert bits_equal(first, real_bits(dev, X, sets, seed, 200))
        monkeypatch.setenv("HIBAG_SCORE_PANEL_PERMS", "16")
        assert bits_equal(first, real_bits(dev, X, sets, seed, 200))
        monkeypatch.setenv("HIBAG_SCORE_PANEL_PERMS", "48")
        assert bits_equal(first, real_bits(dev, X, sets, seed, 200))
        monkeypatch.delenv("HIBAG_SCORE_PANEL_PERMS")
        m1, c1 = dev.score_resample(seed, 1, 100)
        m2, c2 = dev.score_resample(seed, 101, 100)
        assert np.concatenate([m1, m2]).tobytes() == first[-2].tobytes() and np.array_equal(c1 + c2, first[-1])
        assert bits_equal(before, int8_bits(dev, isets, seed, 200))                          # the int8 rows are installed again
        # the first 17 rows alone: the sets within them give the same numbers
        sub = [s for s in sets if all(r < 17 for r in s)]
        pick = [sets.index(s) for s in sub]
        assert len(sub) >= 20 and [] in sub
        alone = real_bits(dev, X[:17], sub, seed, 200)
        whole = real_bits(dev, X, sub, seed, 200)
        whole[0], whole[2 + len(sub)] = whole[0][:17], whole[2 + len(sub)][:17]              # proj and g hold every row
        assert bits_equal(alone, whole)
        assert all(first[2 + t].tobytes() == alone[2 + j].tobytes() for j, t in enumerate(pick))       # S per set
        assert first[3 + len(sets)][pick].tobytes() == alone[3 + len(sub)].tobytes()                   # stat per set
        assert bits_equal(before, int8_bits(dev, isets, seed, 200))


def test_rows_of_0_1_2_agree_with_the_int8_path():
    case, seed = "n1000", SR.seed_of("n1000", "additive")
    A = SR.analysis(case, "additive")[0]
    Zi = SR.reference(case, "additive")
    tol = SR.tolerance(case, "additive")
    rows = 33
    sets = [s for s in Zi.sets if all(r < rows for r in s)]
    assert max(len(s) for s in sets) == 30 and [] in sets
    with open_case(case) as dev:
        a = int8_bits(dev, sets, seed, 129)
        b = real_bits(dev, A.F[:rows].astype(np.float64), sets, seed, 129)
    n = len(sets)
    # kept, df, flags, count_point: integers
    for k in (1, 4 + n, 5 + n, 7 + n):
        assert a[k].dtype.kind == "i" and np.array_equal(a[k], b[k]), k
    scale = SR.numbers(Zi)
    pick = [Zi.sets.index(s) for s in sets]
    got = dict(proj=b[0], S=b[2:2 + n], g=b[2 + n], stat=b[3 + n], max_stat=b[6 + n])
    want = dict(proj=a[0][:rows], S=a[2:2 + n], g=a[2 + n][:rows], stat=a[3 + n], max_stat=a[6 + n],
                srr=scale["srr"][:rows], xx=scale["xx"][:rows], rr=scale["rr"])
    d = SR.differences(got, want)
    print(f"0 / 1 / 2 rows, real against int8: {d} (tol {tol:.3g})")
    assert max(d.values()) <= tol and len(pick) == n


def test_real_sets_reject_invalid_arguments():
    L, p = _lib.lib(), assoc._ptr
    i32 = lambda v: np.array(v, np.int32)      # noqa: E731
    err = L.hibag_hip_last_error
    real = L.hibag_hip_assoc_rscore_sets
    with open_case("n40") as dev:
        n = dev.n_kept
        X = np.random.default_rng(1).uniform(0, 2, (31, n))
        proj, S, kept = np.empty((31, dev.n_basis)), np.empty(31 * 31 + 4), np.empty(4, np.int32)
        start, rows = i32([0, 1, 3]), i32([0, 1, 2])
        outs = (p(proj), p(S), p(kept))
        assert real(dev._s, p(X), 31, p(i32([0, 31])), p(i32(list(range(31)))), 1, *outs) == -1 and b"at most 30" in err()
        assert real(dev._s, p(X), 31, p(i32([0, 30])), p(i32(list(range(30)))), 1, *outs) == 0
        for v in (np.nan, np.inf, -np.inf):
            bad = X.copy()
            bad[2, n - 1] = v
            assert real(dev._s, p(bad), 31, p(start), p(rows), 2, *outs) == -1 and b"finite" in err()
        assert real(dev._s, None, 31, p(start), p(rows), 2, *outs) == -1 and real(None, p(X), 31, p(start), p(rows), 2, *outs) == -1
        assert real(dev._s, p(X), 0, p(start), p(rows), 2, *outs) == -1
        assert real(dev._s, p(X), 2, p(start), p(rows), 2, *outs) == -1 and b"outside" in err()      # row 2 of two rows
        assert real(dev._s, p(X), 31, None, p(rows), 2, *outs) == -1 and real(dev._s, p(X), 31, p(start), None, 2, *outs) == -1
        for k in range(3):
            o = list(outs)
            o[k] = None
            assert real(dev._s, p(X), 31, p(start), p(rows), 2, *o) == -1
        assert real(dev._s, p(X), 31, p(start), p(rows), 2, *outs) == 0 and kept[0] == 1 and kept[1] == 3
        g, stat, df, fl = np.empty(31), np.empty(2), np.empty(2, np.int32), np.empty(2, np.int32)
        assert L.hibag_hip_assoc_score_observed(dev._s, p(g), p(stat), p(df), p(fl)) == 0 and df.tolist() == [1, 2] and np.isfinite(g).all()


# 3 end to end -------------------------------------------------------------------------------------------------------------
def assert_results_close(got, want, tol):
    assert got.name == want.name and np.array_equal(got.flags, want.flags) and np.array_equal(got.df, want.df)
    assert (got.n_samp, got.n_case, got.n_perm, got.seed) == (want.n_samp, want.n_case, want.n_perm, want.seed)
    assert got.base["name"] == want.base["name"] and np.allclose(got.base["est"], want.base["est"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got.freq, want.freq, equal_nan=True) and np.array_equal(got.mean_dosage, want.mean_dosage, equal_nan=True)
    for key in ("score_stat", "score_p") + (("perm_p", "perm_p_adj", "max_stat", "min_p") if want.n_perm else ()):
        assert np.array_equal(np.isnan(getattr(got, key)), np.isnan(getattr(want, key))), key
    assert (want.flags == 0).sum() >= 1
    assert np.nanmax(np.abs(got.score_stat - want.score_stat) / np.fmax(want.score_stat, 1)) <= tol
    fin = np.isfinite(want.score_p)
    assert (np.abs(np.log(got.score_p[fin] / want.score_p[fin])) <= tol * np.fmax(want.score_stat[fin], 1) + 1e-12).all()
    if want.n_perm:
        assert np.array_equal(got.max_stat_df, want.max_stat_df)
        assert np.allclose(got.max_stat, want.max_stat, rtol=tol, atol=tol, equal_nan=True)
        assert np.array_equal(got.perm_p, want.perm_p, equal_nan=True) and np.array_equal(got.perm_p_adj, want.perm_p_adj, equal_nan=True)


def test_hla_assoc_haplo_end_to_end():
    h1, h2, prob, n_allele, y, cov = HR.e2e_cohort()
    n = h1.shape[1]
    ids = [f"s{i}" for i in range(n)]
    calls = {f"L{l}": HlaTopCalls(f"L{l}", list(ids), h1.shape[2], h1[l], h2[l], prob[l], np.ones(n), levels=[f"L{l}*{i:04d}" for i in range(n_allele)])
             for l in range(3)}
    res = hb.hlaHaplotypes(calls, verbose=False, dosage_min_freq=0.01)
    ref, r = HR.haplo_result(h1, h2, prob, n_allele, dosage_min_freq=0.01)
    assert res.keys.tobytes() == ref.keys.tobytes() and np.array_equal(res.dosage_index, ref.dosage_index)
    assert_dosage_bits(res.dosage, ref.dosage, "the cohort's dosages")
    # the tolerance of this design, from the restatement alone
    sel = np.flatnonzero(res.freq >= 0.02)
    at = {int(i): k for k, i in enumerate(res.dosage_index)}
    D = np.ascontiguousarray(res.dosage[[at[int(i)] for i in sel]][:, res.used])
    covT = np.ascontiguousarray(cov[res.used].T)
    sets = [[j] for j in range(len(D))]
    Zs = [HR.RealScore(D, y[res.used], covT, dtype=dt).install(sets) for dt in (np.float64, np.longdouble)]
    for Z in Zs:
        Z.perm_T = Z.stats(HR.E2E_SEED, 1, 200)
        Z.max_stat, Z.count = Z.max_and_count(Z.perm_T)
    tol = HR.tolerance_of(*Zs)
    kw = dict(min_freq=0.02, n_perm=200, seed=HR.E2E_SEED)
    got = hb.hlaAssocHaplo(res, y, cov, **kw)
    assert_results_close(got, hb.hlaAssocHaplo(res, y, cov, _backend=HR.Backend, **kw), tol)
    top = got.name[int(np.nanargmax(got.score_stat))]
    assert top == res.names(0) and got.score_p.min() < 0.01
    cgot = hb.hlaAssocHaplo(res, y, cov, condition=[top], **kw)
    assert cgot.flags[0] & 2 and cgot.base["name"][-1] == f"h[{top}]"
    assert_results_close(cgot, hb.hlaAssocHaplo(res, y, cov, condition=[top], _backend=HR.Backend, **kw), tol)
    ogot = hb.hlaAssocHaplo(res, y, cov, omnibus=True, **kw)
    assert ogot.name == ["omnibus"] and ogot.df[0] == len(sel)
    assert_results_close(ogot, hb.hlaAssocHaplo(res, y, cov, omnibus=True, _backend=HR.Backend, **kw), tol)
    # best: hlaAssocScore on the called pairs, bit for bit
    b = hb.hlaAssocHaplo(res, y, cov, dosage="best", **kw)
    s = hb.hlaAssocScore(res.as_alleles(0.02), y, cov, model="additive", n_perm=200, seed=HR.E2E_SEED)
    pick = [s.name.index(name) for name in b.name]
    for key in ("score_stat", "score_p", "perm_p", "perm_p_adj", "df", "flags"):
        assert np.asarray(getattr(b, key)).tobytes() == np.asarray(getattr(s, key))[pick].tobytes(), key
    assert b.max_stat.tobytes() == s.max_stat.tobytes() and b.dosage == "best"
