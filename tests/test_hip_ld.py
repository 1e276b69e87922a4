"""hlaGenoLD / hlaLDMatrix on the GPU: bit for bit equal to the CPU reference (tests/ld_reference.py), NaN positions
included (the bits are compared), in both memory orders, at sample and SNP counts around the kernels' tile sizes, with
missing data, forced panel splits, and at the 10,000 x 5,000 scale."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ld_reference as R  # noqa: E402

import hibag_amd as hb  # noqa: E402
from hibag_amd.ld import _DeviceGeno, _geno_ld_r2  # noqa: E402

pytestmark = pytest.mark.gpu

NA = hb.NA_INTEGER
LOCI = ("A", "B", "C", "DQA1", "DQB1", "DRB1")


def assert_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape
    diff = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert diff.size == 0, f"{len(diff)} cells differ, first {tuple(diff[0])}: {got[tuple(diff[0])]!r} vs {want[tuple(diff[0])]!r}"


def _orders(g):
    g = np.asarray(g, np.int32)
    return {"snp_major": np.ascontiguousarray(g), "sample_major": np.asfortranarray(g)}


def _geno(g, ids=None):
    n = g.shape[1]
    ids = ids or [f"s{i}" for i in range(n)]
    return hb.HlaSNPGeno(genotype=g, sample_id=ids, snp_id=[f"rs{j}" for j in range(g.shape[0])], assembly="hg19")


def _check_geno_ld(g, a1, a2):
    ids = [f"s{i}" for i in range(g.shape[1])]
    hla = hb.HlaAlleleClass(locus="A", sample_id=ids, allele1=a1, allele2=a2)
    want_ld, want_r2, _ = R.geno_ld(g, a1, a2)
    for order, gg in _orders(g).items():
        ld, r2, _ = _geno_ld_r2(hla, _geno(gg, ids))
        assert_bits(r2, want_r2)
        assert_bits(ld, want_ld)
        assert_bits(hb.hlaGenoLD(hla, _geno(gg, ids)), want_ld)


def _check_ld_matrix(g, maf=0.01):
    keep = R.maf_keep(g, maf)
    want, _ = R.ld_matrix(g[keep])
    for order, gg in _orders(g).items():
        assert_bits(hb.hlaLDMatrix(_geno(gg), maf=maf, draw=False, verbose=False), want)


def _random_case(rng, n_snp, n_samp, n_allele=9, na_geno=0.05, na_hla=0.1):
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.int32)
    g[rng.random(g.shape) < na_geno] = NA
    names = [f"{k:02d}:01" for k in range(n_allele)]
    a1 = [names[i] for i in rng.integers(0, n_allele, n_samp)]
    a2 = [names[i] for i in rng.integers(0, n_allele, n_samp)]
    for s in np.flatnonzero(rng.random(n_samp) < na_hla):
        (a1 if s % 2 else a2)[s] = None
    return g, a1, a2


@pytest.mark.parametrize("locus", LOCI)
def test_geno_ld_fixture(hapmap_geno, hla_type_table, locus):
    a1, a2 = list(hla_type_table[locus + ".1"]), list(hla_type_table[locus + ".2"])
    hla = hb.HlaAlleleClass(locus=locus, sample_id=list(hla_type_table["sample.id"]), allele1=a1, allele2=a2)
    want_ld, want_r2, _ = R.geno_ld(hapmap_geno.genotype, a1, a2)
    assert np.isnan(want_ld).sum() >= 32
    for order, gg in _orders(hapmap_geno.genotype).items():
        geno = hb.HlaSNPGeno(genotype=gg, sample_id=hapmap_geno.sample_id, snp_id=hapmap_geno.snp_id)
        ld, r2, _ = _geno_ld_r2(hla, geno)
        assert_bits(r2, want_r2)
        assert_bits(ld, want_ld)
    # hla in another sample order: reordered to the genotypes' samples (R's match)
    perm = np.random.default_rng(3).permutation(len(a1))
    shuffled = hb.HlaAlleleClass(locus=locus, sample_id=[hla.sample_id[i] for i in perm], allele1=[a1[i] for i in perm],
                                 allele2=[a2[i] for i in perm])
    assert_bits(hb.hlaGenoLD(shuffled, hapmap_geno), want_ld)
    # the numeric-matrix and vector forms
    assert_bits(hb.hlaGenoLD(hla, hapmap_geno.genotype.astype(np.float64)), want_ld)
    assert_bits(hb.hlaGenoLD(hla, hapmap_geno.genotype[5].astype(np.float64)), want_ld[5:6])


@pytest.mark.parametrize("maf", [0.01, 0.0])
def test_ld_matrix_fixture(hapmap_geno, maf):
    _check_ld_matrix(np.asarray(hapmap_geno.genotype), maf)


@pytest.mark.parametrize("n_samp", [1, 2, 31, 32, 33, 63, 64, 65, 4097])
def test_sample_counts(n_samp):
    rng = np.random.default_rng(n_samp)
    for n_snp in (1, 37, 70):
        g, a1, a2 = _random_case(rng, n_snp, n_samp, na_geno=0.02)
        _check_geno_ld(g, a1, a2)
        _check_ld_matrix(g, maf=0.0)
        _check_ld_matrix(g, maf=0.05)


def test_missing_data():
    rng = np.random.default_rng(5)
    g, a1, a2 = _random_case(rng, 131, 97, na_geno=0.01, na_hla=0.2)
    g[7, :] = NA                                   # an all-NA SNP
    g[:, 11] = NA                                  # an all-NA sample
    g[9, :] = 1                                    # a monomorphic SNP
    g[12, 3] = 7                                   # values outside {0, 1, 2} are missing in an HlaSNPGeno
    a1[20] = a2[21] = None
    _check_geno_ld(g, a1, a2)
    want_ld, _, _ = R.geno_ld(g, a1, a2)
    assert np.isnan(want_ld[7]) and np.isnan(want_ld[9])
    gm = np.where(g == 7, NA, g)
    _check_ld_matrix(gm, maf=0.0)                  # the all-NA SNP leaves fewer than two complete samples
    _check_ld_matrix(np.delete(gm, 7, axis=0), maf=0.0)
    _check_ld_matrix(gm, maf=0.01)                 # the MAF filter drops the all-NA SNP
    # no allele at all: every SNP NaN
    ld = hb.hlaGenoLD(hb.HlaAlleleClass(locus="A", sample_id=[f"s{i}" for i in range(97)], allele1=[None] * 97,
                                        allele2=[None] * 97), _geno(g))
    assert np.isnan(ld).all()


def test_flanking_snps_of_hla_a(hapmap_geno, capsys):
    snp = hb.hlaFlankingSNP(hapmap_geno.snp_id, hapmap_geno.snp_position, "A", 500000, assembly="hg19")
    pos = {s: i for i, s in enumerate(hapmap_geno.snp_id)}
    sub = hb.hlaGenoSubset(hapmap_geno, snp_sel=[pos[s] for s in snp])
    g = np.asarray(sub.genotype)
    keep = R.maf_keep(g, 0.01)
    assert 0 < len(keep) < g.shape[0]
    got = hb.hlaLDMatrix(sub, loci=["A"], draw=False)
    assert f"MAF filter (>=0.01), excluding {g.shape[0] - len(keep)} SNP(s)" in capsys.readouterr().out
    assert_bits(got, R.ld_matrix(g[keep])[0])
    assert_bits(hb.hlaLDMatrix(sub, maf=0, draw=False), R.ld_matrix(g)[0])


def test_edge_cases():
    g = np.array([[0, 1, NA, 2], [1, NA, 2, 0], [2, 2, 1, NA]], np.int32)   # no two samples complete over all SNPs
    got = hb.hlaLDMatrix(_geno(g), maf=0, draw=False)
    assert got.shape == (3, 3) and np.isnan(got).all()
    assert_bits(got, R.ld_matrix(g)[0])
    g = np.array([[0, 0, 0, 0, 1], [2, 2, 2, 2, 2]], np.int32)              # MAF 0.1 and 0: nothing is kept at 0.2
    assert hb.hlaLDMatrix(_geno(g), maf=0.2, draw=False, verbose=False).shape == (0, 0)
    with _DeviceGeno(g) as dg:
        n_valid, s = dg.snp_counts()
        assert list(n_valid) == [5, 5] and list(s) == [1, 10]


@pytest.mark.parametrize("rows", ["32", "1000"])
def test_forced_panels(monkeypatch, rows):
    rng = np.random.default_rng(int(rows))
    g = rng.integers(0, 3, (2500, 300)).astype(np.int32)
    g[rng.random(g.shape) < 0.0005] = NA
    want = R.ld_matrix(g)[0]
    monkeypatch.setenv("HIBAG_LD_PANEL_ROWS", rows)
    assert_bits(hb.hlaLDMatrix(_geno(g), maf=0, draw=False), want)
    assert_bits(hb.hlaLDMatrix(_geno(np.asfortranarray(g)), maf=0, draw=False), want)


def test_synthetic_10000_by_5000():
    rng = np.random.default_rng(2024)
    n_snp, n_samp = 5000, 10000
    g = rng.integers(0, 3, (n_snp, n_samp)).astype(np.int32)
    na_samp = rng.choice(n_samp, n_samp * 3 // 100, replace=False)
    g[rng.integers(0, n_snp, na_samp.size), na_samp] = NA                   # NAs in 3 % of the samples
    assert_bits(hb.hlaLDMatrix(_geno(g), maf=0.01, draw=False, verbose=False), R.ld_matrix(g[R.maf_keep(g, 0.01)])[0])
    names = [f"{k:02d}:{k % 7:02d}" for k in range(60)]
    a1 = [names[i] for i in rng.integers(0, 60, n_samp)]
    a2 = [names[i] for i in rng.integers(0, 60, n_samp)]
    a1[17] = None
    _check_geno_ld(g, a1, a2)
