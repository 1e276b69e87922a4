"""hlaPredictDraws on the host: the generator's known answers, the uniform, the definition (tests/draws_reference.py) on
hand-made rows -- frequencies, a zero cell never drawn, NA for rows without mass or with NaN -- the prefix property, and
against the oracle's posterior on the HapMap fixture; and the parts of the feature that need no device: the exported
names, the declared symbols, the checks of `n`, the result object assembled from given arrays."""
import os
import re

import numpy as np
import pytest

import hibag_amd as hb
from conftest import ROOT, align_geno
from draws_reference import draws, draws_from_postprob, draws_from_uniform, philox4x32_10, uniform
from hibag_amd import NA_INTEGER

NA = NA_INTEGER
NAN = float("nan")


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(philox4x32_10([f, f, f, f], [f, f])) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised: rows of counters against one key
    both = philox4x32_10([[0, 0, 0, 0], [1, 0, 0, 0]], [0, 0])
    assert both.shape == (2, 4) and _hex(both[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(both[1]) != _hex(both[0])


def test_uniform_is_in_the_unit_interval_and_depends_on_seed_index_and_draw():
    idx = np.arange(2000, dtype=np.uint64)[:, None]
    t = np.arange(16, dtype=np.uint64)[None, :]
    u = uniform(7, idx, t)
    assert u.shape == (2000, 16) and u.dtype == np.float64 and np.all(u >= 0) and np.all(u < 1)
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
    base = float(uniform(7, 3, 2))
    assert base == u[3, 2]
    assert float(uniform(8, 3, 2)) != base and float(uniform(7 + (1 << 32), 3, 2)) != base           # both halves of the seed
    assert float(uniform(7, 4, 2)) != base and float(uniform(7, 3 + (1 << 32), 2)) != base           # both halves of the index
    assert float(uniform(7, 3, 3)) != base
    w = philox4x32_10([3, 0, 2, 0], [7, 0]).astype(np.uint64)
    assert base == float((int(w[0]) >> 5) * (1 << 26) + (int(w[1]) >> 6)) * 2.0 ** -53


def test_frequencies_follow_the_row_and_a_zero_cell_is_never_drawn():
    #                    cell: (0,0) (0,1) (1,1) ... of 2 alleles would be 3 cells; 4 cells need a free-standing check:
    p = np.array([0.5, 0.3, 0.0, 0.2])
    n_idx, n = 1000, 20
    u = uniform(7, np.arange(n_idx, dtype=np.uint64)[:, None], np.arange(n, dtype=np.uint64)[None, :])
    cum = np.cumsum(p)
    cell = (cum[None, None, :] > (u * cum[-1])[:, :, None]).argmax(axis=2)
    N = n_idx * n
    freq = np.bincount(cell.ravel(), minlength=4) / N
    print("frequencies", freq)
    sigma = np.sqrt(p * (1 - p) / N)
    assert sigma.max() <= 0.0036
    assert np.all(np.abs(freq - p) <= 5 * sigma) and freq[2] == 0
    assert np.allclose(freq, [0.4987, 0.30245, 0, 0.19885], atol=1e-12)
    # the same through the definition: a 6-cell row (3 alleles) with the zero cells in the middle and at the end
    row = np.array([[0.5, 0.3, 0.0, 0.2, 0.0, 0.0]])
    r = draws_from_uniform(np.repeat(row, n_idx, axis=0), u, 3)
    got = r["h2"] + r["h1"] * (2 * 3 - r["h1"] - 1) // 2
    assert np.array_equal(got, cell)
    assert np.array_equal(r["prob"], row[0][cell])


def test_single_cell_zero_rows_and_nan_rows():
    pp = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0],        # one positive cell: (1, 1)
                   [0.0] * 6,
                   [0.2, NAN, 0.3, 0.0, 0.0, 0.5],
                   [NAN] * 6,
                   [0.0, 0.0, 0.0, 0.0, 0.0, 3e-300]])    # a tiny total is a total
    r = draws_from_postprob(pp, 9, seed=5, sample0=0, n_hla=3)
    assert r["h1"].dtype == np.int32 and r["prob"].shape == (5, 9)
    assert np.all(r["h1"][0] == 1) and np.all(r["h2"][0] == 1) and np.all(r["prob"][0] == 1.0)
    assert np.all(r["h1"][1] == NA) and np.all(r["h2"][1] == NA) and np.all(r["prob"][1] == 0.0)
    for s in (2, 3):
        assert np.all(r["h1"][s] == NA) and np.all(r["h2"][s] == NA) and np.isnan(r["prob"][s]).all()
    assert np.all(r["h1"][4] == 2) and np.all(r["h2"][4] == 2) and np.all(r["prob"][4] == 3e-300)
    # no cell qualifies (u * S rounds up to S): the last positive cell
    f = draws_from_uniform(np.array([[0.25, 0.75, 0.0]]), np.array([[1.0]]), 2)
    assert (f["h1"][0, 0], f["h2"][0, 0], f["prob"][0, 0]) == (0, 1, 0.75)


def test_prefix_property_and_sample0_on_the_reference():
    rng = np.random.default_rng(3)
    pp = rng.random((40, 10)) * (rng.random((40, 10)) < 0.6)
    big = draws_from_postprob(pp, 33, seed=99, sample0=0, n_hla=4)
    small = draws_from_postprob(pp, 5, seed=99, sample0=0, n_hla=4)
    for key in ("h1", "h2", "prob"):
        assert np.array_equal(big[key][:, :5], small[key]), key
    part = draws_from_postprob(pp[11:29], 33, seed=99, sample0=11, n_hla=4)
    unshifted = draws_from_postprob(pp[11:29], 33, seed=99, sample0=0, n_hla=4)
    for key in ("h1", "h2", "prob"):
        assert np.array_equal(big[key][11:29], part[key]), key
    assert not np.array_equal(big["h1"][11:29], unshifted["h1"])
    assert not np.array_equal(big["h1"], draws_from_postprob(pp, 33, seed=100, sample0=0, n_hla=4)["h1"])


def test_draws_from_the_oracles_posterior_on_the_hapmap_fixture(model_a, hapmap_geno, oracle):
    G = align_geno(model_a, hapmap_geno, hapmap_geno.sample_id)
    n_hla = model_a.n_hla
    for vote in (1, 2):
        r = draws(model_a, G, 12, seed=2024, vote=vote)
        ok = r["h1"][:, 0] != NA
        assert ok.any() and np.array_equal(ok, r["call"]["h1"] != NA)
        cell = r["h2"][ok].astype(np.int64) + r["h1"][ok].astype(np.int64) * (2 * n_hla - r["h1"][ok] - 1) // 2
        val = np.take_along_axis(r["postprob"][ok], cell, axis=1)
        assert np.all(val > 0) and np.array_equal(val, r["prob"][ok])
        assert np.all(r["h1"][ok] <= r["h2"][ok]) and np.all(r["h1"][ok] >= 0) and np.all(r["h2"][ok] < n_hla)
        assert np.all(r["h1"][~ok] == NA) and np.all(r["h2"][~ok] == NA)


def test_names_are_exported():
    assert "hlaPredictDraws" in hb.__all__ and "HlaPosteriorDraws" in hb.__all__
    assert callable(hb.hlaPredictDraws) and isinstance(hb.HlaPosteriorDraws, type)
    for name in ("predict_draw", "predict_draw_mapped", "predict_draw_snp_major", "predict_draw_bed", "predict_draw_device",
                 "predict_draw_cohort"):
        assert hasattr(hb.HlaAttrBagClass, name), name


DRAW_ENTRIES = ["hibag_hip_predict_draw", "hibag_hip_predict_draw_device", "hibag_hip_predict_draw_mapped",
                "hibag_hip_predict_draw_snp_major", "hibag_hip_predict_draw_bed", "hibag_hip_predict_draw_cohort"]


def test_symbols_are_declared_and_exported():
    from hibag_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hibag_hip.h")).read()
    declared = set(re.findall(r"\b(hibag_hip_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in DRAW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    m = re.search(r"#define\s+HIBAG_HIP_DRAW_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.DRAW_MAX == 64
    assert re.search(r"#define\s+HIBAG_HIP_ABI_VERSION\s+7\b", hdr) and "within version 7" in hdr
    # two more arguments (seed, sample0) than the sibling top-k entry
    for suffix in ("", "_device", "_mapped", "_snp_major", "_bed", "_cohort"):
        assert len(getattr(L, "hibag_hip_predict_draw" + suffix).argtypes) \
            == len(getattr(L, "hibag_hip_predict_topk" + suffix).argtypes) + 2, suffix


def _shell(obj):
    """An hlaAttrBagClass without a device model: enough for the checks that come before any device work."""
    m = object.__new__(hb.HlaAttrBagClass)
    m.obj, m._h = obj, None
    return m


def test_n_is_checked_before_any_device_work(model_a):
    from hibag_amd import _lib
    from hibag_amd.hibag import draw_n
    assert draw_n(1) == 1 and draw_n(np.int32(_lib.DRAW_MAX)) == _lib.DRAW_MAX and draw_n(4.0) == 4
    G = np.zeros((model_a.n_snp, 3), np.int32)
    m = _shell(model_a)
    for bad in (0, _lib.DRAW_MAX + 1, -1, 2.5, "3", None, True):
        with pytest.raises(ValueError, match=str(_lib.DRAW_MAX)):
            draw_n(bad)
        with pytest.raises(ValueError, match=str(_lib.DRAW_MAX)):
            hb.hlaPredictDraws(m, G, n=bad, seed=1, verbose=False)
        with pytest.raises(ValueError, match=str(_lib.DRAW_MAX)):
            m.predict_draw(G.T, bad, 1)
    with pytest.raises(ValueError, match="sample0"):
        m.predict_draw(G.T, 3, 1, sample0=-1)
    with pytest.raises(ValueError, match="seed"):
        hb.hlaPredictDraws(m, G, n=3, seed=1.5, verbose=False)
    with pytest.raises(TypeError):
        hb.hlaPredictDraws(model_a, G, verbose=False)             # an hlaAttrBagObj is not a device model
    with pytest.raises(ValueError):
        hb.hlaPredictDraws(m, G, vote="mean", verbose=False)
    with pytest.raises(TypeError):
        hb.hlaPredictDraws(m, G, cl=[0], verbose=False)           # several devices: not part of this function
    with pytest.raises(TypeError):
        hb.hlaPredictDraws(m, np.array([["a"] * 3] * model_a.n_snp), seed=1, verbose=False)
    with pytest.raises(ValueError):
        hb.hlaPredictDraws(m, G[:-1], seed=1, verbose=False)


def test_the_result_object(model_a):
    al = model_a.hla_allele
    h1 = np.array([[0, 1, 0], [2, 2, 3], [NA, NA, NA]], np.int32)
    h2 = np.array([[1, 1, 1], [3, 3, 3], [NA, NA, NA]], np.int32)
    prob = np.array([[0.6, 0.3, 0.6], [0.7, 0.7, 0.2], [0.0, 0.0, 0.0]])
    mt = np.array([0.5, 0.25, NAN])
    ids = ["a", "b", "c"]
    d = hb.HlaPosteriorDraws(model_a.hla_locus, ids, 3, h1, h2, prob, mt, seed=17, assembly="hg19", levels=al)
    assert d.n == 3 and len(d) == 3 and d.seed == 17 and d.locus == model_a.hla_locus and d.sample_id == ids
    assert d.assembly == "hg19" and d.levels == al and "n=3" in repr(d)
    assert d.allele1 == [[al[0], al[2], None], [al[1], al[2], None], [al[0], al[3], None]]
    assert d.allele2 == [[al[1], al[3], None], [al[1], al[3], None], [al[1], al[3], None]]
    one = d.draw(1)
    assert isinstance(one, hb.HlaAlleleClass) and np.array_equal(one.h1, h1[:, 1]) and np.array_equal(one.h2, h2[:, 1])
    assert np.array_equal(one.prob, prob[:, 1]) and one.matching is mt and one.sample_id == ids and one.assembly == "hg19"
    assert one.allele1 == [al[1], al[2], None] and one.dosage is None and one.postprob is None
    every = list(d)
    assert len(every) == 3 and all(isinstance(x, hb.HlaAlleleClass) for x in every)
    assert [x.allele2 for x in every] == d.allele2
    true = hb.HlaAlleleClass(locus=model_a.hla_locus, sample_id=ids, allele1=[al[1], al[0], al[0]], allele2=[al[1], al[0], al[0]])
    assert hb.hlaCompareAllele(true, one)["total.num.ind"] == 2
    for bad in (3, -1, 1.0, True):
        with pytest.raises(IndexError):
            d.draw(bad)
    with pytest.raises(ValueError):
        hb.HlaPosteriorDraws(model_a.hla_locus, ids, 2, h1, h2, prob, mt, levels=al)
    with pytest.raises(ValueError):
        hb.HlaPosteriorDraws(model_a.hla_locus, ids[:2], 3, h1, h2, prob, mt, levels=al)
