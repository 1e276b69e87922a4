"""The host side of hlaPredictMerge: the merge plan (the name work of hlaPredMerge as one function), the plain-loop yardstick
of the merge arithmetic (tests/predmerge_reference.py) pinned to the shipped hlaPredMerge, and the argument errors of
hlaPredictMerge that need no device."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predmerge_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd import synth  # noqa: E402
from hibag_amd.hibag import HlaAlleleClass, HlaAttrBagClass, _pair_names  # noqa: E402
from hibag_amd.merge import merge_plan  # noqa: E402

A1 = ["01:01", "01:02", "02:01:01G", "02:05", "03:01N", "24:02"]
A2 = ["01:02", "02:01:02", "02:05", "11:01", "24:02", "24:03Q", "68:01"]
EQUIV = {"24:03Q": "24:02", "11:01": "03:01N"}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_plan(lists, plan, replace):
    """`plan` against the names: `replace` is the per-allele replacement the options stand for."""
    merged = hb.hlaUniqueAllele([replace(a) for al in lists for a in al])
    assert plan.hla_allele == merged
    n = len(merged)
    P = n * (n + 1) // 2
    assert plan.pair_names == _pair_names(merged) and plan.n_row == P
    row = {nm: r for r, nm in enumerate(plan.pair_names)}
    seen = set()
    for m, al in enumerate(lists):
        src = _pair_names(al)
        assert plan.row_of_cell[m].dtype == np.int32 and len(plan.row_of_cell[m]) == len(src)
        for j, nm in enumerate(src):
            a, b = (replace(x) for x in nm.split("/"))
            want = row.get(f"{a}/{b}", row.get(f"{b}/{a}"))
            assert want is not None and plan.row_of_cell[m][j] == want, (m, nm)
    # gather lists: sorted (model, cell) per row, every source cell exactly once, in its own row
    assert len(plan.gather_off) == P + 1 and plan.gather_off[0] == 0 and plan.gather_off[-1] == len(plan.gather_cell)
    for r in range(P):
        ent = [(int(plan.gather_model[e]), int(plan.gather_cell[e])) for e in range(plan.gather_off[r], plan.gather_off[r + 1])]
        assert ent == sorted(ent)
        for m, j in ent:
            assert plan.row_of_cell[m][j] == r
            assert (m, j) not in seen
            seen.add((m, j))
    assert len(seen) == sum(len(al) * (len(al) + 1) // 2 for al in lists)
    # dosage lists: every row exactly twice, a diagonal row in both lists of its allele
    count = np.zeros(P, int)
    for a in range(n):
        first = plan.first_rows[plan.first_off[a]:plan.first_off[a + 1]]
        second = plan.second_rows[plan.second_off[a]:plan.second_off[a + 1]]
        assert list(first) == sorted(first) and list(second) == sorted(second)
        assert all(plan.pair_names[r].split("/")[0] == merged[a] for r in first)
        assert all(plan.pair_names[r].split("/")[1] == merged[a] for r in second)
        assert row[f"{merged[a]}/{merged[a]}"] in first and row[f"{merged[a]}/{merged[a]}"] in second
        np.add.at(count, first, 1)
        np.add.at(count, second, 1)
    assert (count == 2).all()
    return plan


def test_plan_partial_overlap():
    plan = check_plan([A1, A2], merge_plan([A1, A2]), lambda a: a)
    assert len(plan.hla_allele) == 10                     # 6 + 7 - 3 shared
    assert max(np.diff(plan.gather_off)) == 2 and min(np.diff(plan.gather_off)) == 0      # cross-model pairs have no source
    for r in plan.row_of_cell:
        assert len(set(r.tolist())) == len(r)             # one-to-one without a replacement


def test_plan_many_to_one():
    def replace(a):
        return hb.hlaAlleleDigit([EQUIV.get(a, a)], "2-digit", True)[0]
    plan = check_plan([A1, A2], merge_plan([A1, A2], equivalence=EQUIV, max_resolution="2-digit", rm_suffix=True), replace)
    assert plan.hla_allele == ["01", "02", "03", "24", "68"]
    assert any(len(set(r.tolist())) < len(r) for r in plan.row_of_cell)      # many-to-one
    assert max(np.diff(plan.gather_off)) > 2                                   # gather lists longer than k
    check_plan([A1, A2, A1[:3]], merge_plan([A1, A2, A1[:3]], equivalence=EQUIV), lambda a: EQUIV.get(a, a))


def random_predictions(lists, n_samp, seed):
    rng = np.random.default_rng(seed)
    pds = []
    for al in lists:
        P = len(al) * (len(al) + 1) // 2
        pp = rng.random((P, n_samp)) ** 4
        pp[rng.random((P, n_samp)) < 0.3] = 0.0
        pp /= pp.sum(axis=0)
        mt = rng.random(n_samp) * 1e-3
        pds.append(HlaAlleleClass(locus="A", sample_id=list(range(n_samp)), allele1=[None] * n_samp, allele2=[None] * n_samp,
                                  prob=np.zeros(n_samp), matching=mt, postprob=pp, pair_names=_pair_names(al), assembly="hg19"))
    return pds


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("use_matching", [True, False])
def test_reference_is_hlaPredMerge(k, use_matching):
    """The yardstick restates what ships: bit-equal to hlaPredMerge on random posteriors (cohorts of >= 2 samples: with one
    sample numpy sums hlaPredMerge's dosage pairwise)."""
    lists = [A1, A2, A1[1:5] + ["68:01"], A2[::2]][:k]
    weight = None if k != 2 else [0.3, 1.9]
    for n_samp, opts in ((2, {}), (7, {}), (5, dict(equivalence=EQUIV, max_resolution="4-digit", rm_suffix=True))):
        pds = random_predictions(lists, n_samp, 100 * k + n_samp)
        want = hb.hlaPredMerge(*pds, weight=weight, use_matching=use_matching, ret_postprob=True, verbose=False, **opts)
        plan = merge_plan(lists, **opts)
        got = R.merge_reference([p.postprob for p in pds], [p.matching for p in pds], weight, plan.row_of_cell,
                                len(plan.hla_allele), use_matching)
        assert plan.hla_allele == hb.hlaUniqueAllele([a for nm in want.pair_names for a in nm.split("/")])
        assert plan.pair_names == want.pair_names
        for f in ("prob", "matching", "dosage", "postprob"):
            assert same_bits(got[f], getattr(want, f)), (f, n_samp)
        assert np.array_equal(got["h1"], want.h1) and np.array_equal(got["h2"], want.h2)


def test_reference_nan_column():
    """A column of zeros (a sample no model could type): total 0, every posterior NaN, the call is row 0 with a NaN prob."""
    pds = random_predictions([A1, A2], 3, 5)
    for p in pds:
        p.postprob[:, 1] = 0.0
    want = hb.hlaPredMerge(*pds, ret_postprob=True, verbose=False)
    plan = merge_plan([A1, A2])
    got = R.merge_reference([p.postprob for p in pds], [p.matching for p in pds], None, plan.row_of_cell, len(plan.hla_allele))
    assert np.isnan(got["prob"][1]) and got["h1"][1] == 0 and got["h2"][1] == 0
    for f in ("prob", "matching", "dosage", "postprob"):
        assert same_bits(got[f], getattr(want, f)), f
    assert np.array_equal(got["h1"], want.h1) and np.array_equal(got["h2"], want.h2)


def fake_model(locus="A", alleles=None):
    """An HlaAttrBagClass without a device handle: enough for the checks that come before any device work."""
    obj, _, _ = synth.make_model("hla-a-small", n_classifier=1)
    obj.hla_locus = locus
    if alleles is not None:
        obj.hla_allele = alleles
    m = object.__new__(HlaAttrBagClass)
    m.obj = obj
    m._h = None
    return m


def test_argument_errors():
    m1, m2 = fake_model(), fake_model()
    g = np.zeros((m1.obj.n_snp, 3), np.int32)
    with pytest.raises(ValueError, match=r"No hlaAlleleClass object passed to 'hlaPredMerge\(\)'\."):
        hb.hlaPredictMerge([], g, verbose=False)
    with pytest.raises(TypeError, match="hlaAttrBagClass"):
        hb.hlaPredictMerge([m1, m1.obj], g, verbose=False)
    with pytest.raises(TypeError, match="hlaAttrBagClass"):
        hb.hlaPredictMerge(m1, g, verbose=False)
    with pytest.raises(ValueError, match="The locus should be the same."):
        hb.hlaPredictMerge([m1, fake_model("B")], g, verbose=False)
    with pytest.raises(ValueError, match="Invalid 'weight'."):
        hb.hlaPredictMerge([m1, m2], g, weight=[1.0], verbose=False)
    with pytest.raises(ValueError, match="'weight' should not have NA/NaN."):
        hb.hlaPredictMerge([m1, m2], g, weight=[1.0, float("nan")], verbose=False)
    with pytest.raises(ValueError, match="'weight' should not have a negative value."):
        hb.hlaPredictMerge([m1, m2], g, weight=[1.0, -0.5], verbose=False)
    with pytest.raises(ValueError, match="'arg' should be one of \"prob\", \"majority\""):
        hb.hlaPredictMerge([m1, m2], g, vote="both", verbose=False)
    with pytest.raises(ValueError, match="'max.resolution' should be one of"):
        hb.hlaPredictMerge([m1, m2], g, max_resolution="5-digit", verbose=False)
    with pytest.raises(TypeError, match="is.numeric"):
        hb.hlaPredictMerge([m1, m2], np.array([["a"] * 3] * m1.obj.n_snp), verbose=False)
    with pytest.raises(ValueError, match="nrow\\(snp\\) == object\\$n.snp is not TRUE"):
        hb.hlaPredictMerge([m1, m2], g[:-1], verbose=False)
    # the same messages as the two functions it stands for
    pds = random_predictions([A1, A2], 2, 1)
    for bad in ([1.0], [1.0, float("nan")], [1.0, -0.5]):
        with pytest.raises(ValueError) as e1:
            hb.hlaPredMerge(*pds, weight=bad, verbose=False)
        with pytest.raises(ValueError) as e2:
            hb.hlaPredictMerge([m1, m2], g, weight=bad, verbose=False)
        assert str(e1.value) == str(e2.value)
