"""hlaGenoLD / hlaLDMatrix on the host: the CPU reference (tests/ld_reference.py) against literal restatements of R's
cor(...)^2 and against exact rationals, and the Python-side argument checks (raised before any device work)."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402

LOCI = ("A", "B", "C", "DQA1", "DQB1", "DRB1")


def _hla(table, locus):
    return list(table[locus + ".1"]), list(table[locus + ".2"])


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("locus", LOCI)
def test_geno_ld_reference_matches_literal_cor(hapmap_geno, hla_type_table, locus):
    assert list(hla_type_table["sample.id"]) == list(hapmap_geno.sample_id)
    a1, a2 = _hla(hla_type_table, locus)
    ld, r2, alleles = R.geno_ld(hapmap_geno.genotype, a1, a2)
    ld_l, r2_l = R.geno_ld_literal(hapmap_geno.genotype, a1, a2)
    assert _same_nan(ld, ld_l) and _same_nan(r2, r2_l)
    assert np.nanmax(np.abs(ld - ld_l)) <= 1e-15
    assert np.nanmax(np.abs(r2 - r2_l)) <= 4e-15
    assert np.isnan(ld).sum() >= 32                       # the monomorphic SNPs of the fixture
    assert np.nanmin(r2) >= 0 and np.nanmax(r2) <= 1


@pytest.mark.parametrize("locus", ("A", "DRB1"))
def test_geno_ld_reference_is_the_rounded_rational(hapmap_geno, hla_type_table, locus):
    a1, a2 = _hla(hla_type_table, locus)
    alleles, i1, i2 = R.hla_indices(a1, a2)
    sums = R.geno_ld_sums(hapmap_geno.genotype, i1, i2, len(alleles))
    r2 = R.r2_formula(*sums)
    rng = np.random.default_rng(7)
    cells = zip(rng.integers(0, r2.shape[0], 400), rng.integers(0, r2.shape[1], 400))
    for j, a in cells:
        exact = R.r2_exact(*(s[j, a] for s in sums))
        if exact is None:
            assert math.isnan(r2[j, a])
            continue
        got = r2[j, a]
        assert abs(got - float(exact)) <= 2.0 ** -50 * float(exact) + 1e-300
        # exactly 1 where the integers say so
        if exact == 1:
            assert got == 1.0


def test_ld_matrix_reference_matches_literal_cor(hapmap_geno):
    g = hapmap_geno.genotype
    keep = R.maf_keep(g, 0.01)
    r2, n = R.ld_matrix(g[keep])
    assert n == 27                                      # complete over every kept SNP
    sub = keep[:240]
    r2s, _ = R.ld_matrix(g[sub])
    lit = R.ld_matrix_literal(g[sub])
    assert _same_nan(r2s, lit)
    assert np.nanmax(np.abs(r2s - lit)) <= 1e-15
    assert np.all(np.diag(r2) == 1.0)
    np.testing.assert_array_equal(r2, r2.T)


def test_ld_matrix_reference_is_the_rounded_rational(hapmap_geno):
    g = hapmap_geno.genotype[R.maf_keep(hapmap_geno.genotype, 0.01)]
    r2, n = R.ld_matrix(g)
    complete = ((g == 0) | (g == 1) | (g == 2)).all(axis=0)
    X = g[:, complete].astype(np.int64)
    rng = np.random.default_rng(11)
    for i, j in zip(rng.integers(0, len(g), 300), rng.integers(0, len(g), 300)):
        if i == j:
            continue
        exact = R.r2_exact(n, X[i] @ X[j], X[i].sum(), X[j].sum(), X[i] @ X[i], X[j] @ X[j])
        if exact is None:
            assert math.isnan(r2[i, j])
        else:
            assert abs(r2[i, j] - float(exact)) <= 2.0 ** -50 * float(exact) + 1e-300


def test_ld_matrix_reference_edge_rules():
    g = np.array([[0, 1, 2, hb.NA_INTEGER], [1, 1, 1, 0], [2, 0, 1, 1]], np.int32)
    r2, n = R.ld_matrix(g)
    assert n == 3
    assert np.all(np.diag(r2) == 1.0)                   # SNP 1 is constant over the complete samples: diagonal 1 ...
    assert np.isnan(r2[1, 0]) and np.isnan(r2[1, 2])    # ... the rest NaN
    r2, n = R.ld_matrix(np.array([[0, hb.NA_INTEGER], [1, 2]], np.int32))
    assert n == 1 and np.isnan(r2).all()


# ---- argument checks (no device needed: they come first) ----

def test_geno_ld_sample_mismatch(hapmap_geno, hla_type_table):
    a1, a2 = _hla(hla_type_table, "A")
    ids = list(hla_type_table["sample.id"])
    hla = hb.HlaAlleleClass(locus="A", sample_id=ids[:-1] + ["nobody"], allele1=a1, allele2=a2)
    with pytest.raises(ValueError, match="of geno is not in hla"):
        hb.hlaGenoLD(hla, hapmap_geno)
    short = hb.HlaAlleleClass(locus="A", sample_id=ids[:-1], allele1=a1[:-1], allele2=a2[:-1])
    with pytest.raises(ValueError, match=r"length\(geno\$sample.id\)"):
        hb.hlaGenoLD(short, hapmap_geno)
    with pytest.raises(ValueError, match=r"dim\(geno\)\[2L\]"):
        hb.hlaGenoLD(short, np.zeros((3, 60)))
    with pytest.raises(TypeError, match="hlaAlleleClass"):
        hb.hlaGenoLD(object(), hapmap_geno)
    with pytest.raises(TypeError, match="hlaSNPGenoClass"):
        hb.hlaGenoLD(hla, "geno")


@pytest.mark.parametrize("bad", [3, -1, 0.5, 1.25, np.inf])
def test_geno_ld_values_outside_0_1_2(hla_type_table, bad):
    a1, a2 = _hla(hla_type_table, "A")
    hla = hb.HlaAlleleClass(locus="A", sample_id=list(hla_type_table["sample.id"]), allele1=a1, allele2=a2)
    g = np.zeros((4, 60))
    g[2, 17] = bad
    with pytest.raises(ValueError, match="genotypes must be 0, 1, 2 or NA"):
        hb.hlaGenoLD(hla, g)
    with pytest.raises(ValueError, match="genotypes must be 0, 1, 2 or NA"):
        hb.hlaGenoLD(hla, g[2])


def test_ld_matrix_argument_checks(hapmap_geno):
    with pytest.raises(ValueError, match="'loci' should be one of MHC, A, B, C"):
        hb.hlaLDMatrix(hapmap_geno, loci=["A", "NOT_A_GENE"], draw=False)
    with pytest.raises(ValueError, match="'loci' should be one of"):
        hb.hlaLDMatrix(hapmap_geno, loci="NOPE", draw=False)
    with pytest.raises(NotImplementedError, match="no plotting"):
        hb.hlaLDMatrix(hapmap_geno, draw=True)
    with pytest.raises(TypeError, match="hlaSNPGenoClass"):
        hb.hlaLDMatrix(hapmap_geno.genotype, draw=False)
    with pytest.raises(TypeError, match="is.numeric"):
        hb.hlaLDMatrix(hapmap_geno, maf="0.01", draw=False)
    assert hb.hlaLDMatrix(hb.HlaSNPGeno(genotype=np.zeros((0, 5), np.int32), sample_id=list("abcde"), snp_id=[]),
                          draw=False).shape == (0, 0)


def test_ld_entries_are_declared():
    from hibag_amd import _lib
    for name in ("hibag_hip_ld_geno_new", "hibag_hip_ld_geno_free", "hibag_hip_ld_snp_counts", "hibag_hip_ld_matrix",
                 "hibag_hip_ld_hla", "hibag_hip_ld_gram_ms"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
