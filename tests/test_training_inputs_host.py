"""Properties of the constructed training inputs (tests/training_reference.py), checked with the oracle alone, for
every case the GPU tests of the training scoring kernels run (tests/test_hip_training.py, tests/test_hip_train_scoring.py).
A case that fails one of these could pass on the GPU while checking nothing:

* degenerate share -- a sample whose oracle total is 0 or which has no best guess says nothing about the arithmetic; at
  most 10 % of a case's samples may be such (a cap).  The one exempt case of each form holds exactly one deliberately far
  sample, total 0, so that the NaN / no-guess path is pinned as well;
* top-word sensitivity -- for n_snp > 32 the same inputs scored on the first 32 (nw - 1) SNPs only must give another
  out-of-bag count or another best guess, or a kernel that ignored the last word would pass;
* missing values -- raw genotype values outside 0..2 are missing.
"""

import numpy as np
import pytest

import training_reference as T


def _structure(lst, n_snp):
    """What the issue asks of a haplotype list."""
    assert np.all(np.diff(lst.allele) >= 0) and lst.bits.shape == (len(lst.allele), n_snp)
    lens = lst.lens
    assert np.sum(lens == 0) >= 2, "empty rows"
    assert np.sum(lens == 1) >= 1, "an allele with exactly one haplotype"
    assert np.all(lst.freq > 0) and abs(lst.freq.sum() - 1) > 1e-3, "positive, not normalised"
    # the packed form: the clean bits below n_snp, garbage in both words above
    clean = T.pack_bits(lst.bits)
    full = (1 << 128) - 1
    low = (1 << n_snp) - 1
    as_int = lambda p: [int(r[0]) | (int(r[1]) << 64) for r in p]
    got, want = as_int(lst.packed), as_int(clean)
    assert all((g & low) == w for g, w in zip(got, want))
    if n_snp < 128:
        tail = [g & (full ^ low) for g in got]
        assert any(t >> n_snp & 1 for t in tail) and any(t for t in tail)
        if n_snp <= 64:
            assert any(int(r[1]) != 0 for r in lst.packed), "the unused packed[1] carries garbage"
    if n_snp > 32:
        # two alleles whose haplotypes differ only in bits of the top word
        lo = T.top_word_start(n_snp)
        present = np.where(lens > 0)[0]
        x, y = lst.bits[lst.allele == present[-2]], lst.bits[lst.allele == present[-1]]
        assert {r[:lo].tobytes() for r in x} == {r[:lo].tobytes() for r in y}
        assert {r.tobytes() for r in x}.isdisjoint({r.tobytes() for r in y})


def _degenerate(sc):
    return (sc.total == 0) | (sc.best[:, 0] == T.NA)


def _check_scores(key, lst, geno, a1, a2, boot, far, exempt):
    n_snp, n = lst.n_snp, len(boot)
    sc = T.score(lst, geno, a1, a2, boot, with_total=True)
    deg = _degenerate(sc)
    if exempt:
        assert list(np.where(deg)[0]) == [far], key
        assert sc.total[far] == 0 and sc.best[far, 0] == T.NA and boot[far] == 0
    else:
        assert far < 0 and deg.sum() <= n // 10, (key, int(deg.sum()))
    # every in-bag sample's true alleles have haplotypes (the host insists: src/LibHLA.cpp:1066-1072)
    lens = lst.lens
    assert all(lens[a1[s]] > 0 and lens[a2[s]] > 0 for s in range(n) if boot[s] > 0)
    assert np.isfinite(sc.loss_ib)
    if n_snp > 32:
        cut = T.score(lst, geno, a1, a2, boot, n_snp=T.top_word_start(n_snp), with_total=True)
        assert cut.acc_oob != sc.acc_oob or not np.array_equal(cut.best, sc.best), \
            f"{key}: the top word decides nothing -- a kernel that ignored it would pass"
    return sc


@pytest.mark.parametrize("key", list(T.PLUGIN_CASES))
def test_plugin_case(key, oracle):
    cs = T.plugin_case(key)
    n_snp = cs.lst.n_snp
    _structure(cs.lst, n_snp)
    assert len(cs.lst.allele) <= 40
    n = len(cs.boot)
    if n > 1:
        assert (cs.boot == 0).any() and (cs.boot > 0).any()
        assert (cs.a1 > cs.a2).any() and (cs.a1 <= cs.a2).any(), "the true pair in either order"
    assert set(np.unique(cs.geno)) <= {0, 1, 2, T.NA}
    sc = _check_scores(key, cs.lst, cs.geno, cs.a1, cs.a2, cs.boot, cs.far, key in T.EXEMPT)
    # the shared expected values are these
    ref = T.case_score(key)
    assert ref.acc_oob == sc.acc_oob and ref.loss_ib == sc.loss_ib


@pytest.mark.parametrize("key", list(T.MATCH_CASES))
def test_match_case(key, oracle):
    """The case is past build_haplomatch's pair bound -- or it would run the path every other case runs --, every in-bag
    sample has pairs to return, and its scores say something."""
    cs = T.match_case(key)
    assert T.match_bound(cs) > 1 << 20
    inbag = np.where(cs.boot > 0)[0]
    pairs = T.haplo_matches(cs)
    assert len(inbag) >= 1 and len(pairs) == len(inbag) and all(len(p) >= 1 for p in pairs)
    assert (cs.boot == 0).any() and (cs.a1 > cs.a2).any() and (cs.a1 <= cs.a2).any()
    sc = _check_scores(key, cs.lst, cs.geno, cs.a1, cs.a2, cs.boot, cs.far, False)
    ref = T.match_score(key)
    assert ref.acc_oob == sc.acc_oob and ref.loss_ib == sc.loss_ib


@pytest.mark.parametrize("key", list(T.BATCH_CASES))
def test_batch_case(key, oracle):
    b = T.batch_case(key)
    kw = dict(T.BATCH_CASES[key])
    assert len(b.lists) == kw["n_cand"] and b.columns.shape == (kw["n_cand"], len(b.boot))
    assert np.all(b.base[:, b.n_snp - 1] == T.NA), "the candidate's position is missing in the base genotype"
    assert (b.boot == 0).any() and (b.boot > 0).any()
    for c, lst in enumerate(b.lists):
        _structure(lst, b.n_snp)
        assert {0, 1, 2, T.NA, 3, -1} <= set(np.unique(b.columns[c])), "every raw code"
        _check_scores(f"{key}[{c}]", lst, b.geno(c), b.a1, b.a2, b.boot, b.far, key in T.EXEMPT)
    # one bit longer than a common parent list: without the last bit every candidate's haplotypes are the parent's
    parents = [{(int(a), r[:-1].tobytes()) for a, r in zip(l.allele, l.bits)} for l in b.lists]
    union = set().union(*parents)
    assert all(len(p) >= 0.7 * len(union) for p in parents if key != "direct")
    if key == "direct":
        assert [len(l.allele) for l in b.lists] == [1100, 40] and parents[1] < parents[0]
        assert np.sum(b.lists[0].lens > 0) == 4
    if key.startswith("cells-p"):
        p = kw["n_hla"] - 2
        assert all(np.sum(l.lens > 0) == p and l.lens.max() <= 2 for l in b.lists)


def test_out_of_range_values_are_missing(oracle):
    """NA_INTEGER, 3 and -1 in a raw column give the same planes -- (0, 1) at that position -- and the same scores."""
    b = T.batch_case("snp65")
    g = b.geno(0)
    pos = b.n_snp - 1
    planes = []
    for v in (T.NA, 3, -1, 7, -2147483647):
        h = g.copy()
        h[:, pos] = v
        s1, s2 = T.encode(h)
        assert np.all((s1[:, pos >> 6] >> np.uint64(pos & 63)) & np.uint64(1) == 0)
        assert np.all((s2[:, pos >> 6] >> np.uint64(pos & 63)) & np.uint64(1) == 1)
        planes.append((s1, s2))
    assert all(np.array_equal(p[0], planes[0][0]) and np.array_equal(p[1], planes[0][1]) for p in planes)
    assert np.array_equal(planes[0][0], b.s1) and np.array_equal(planes[0][1], b.s2), "the base genotype is that"
    # and a value in range is not
    h = g.copy()
    h[:, pos] = 1
    assert not np.array_equal(T.encode(h)[0], b.s1)


def test_floor_rule_of_the_expected_values():
    """batch_expected: a loss only where the count reaches the running maximum that starts at the floor."""
    sc = T.batch_scores("snp65")
    acc, loss = T.batch_expected("snp65", 0)
    assert list(acc) == [s.acc_oob for s in sc]
    run = 0
    for c, s in enumerate(sc):
        assert loss[c] == (s.loss_ib if s.acc_oob >= run else 0.0)
        run = max(run, s.acc_oob)
    acc2, loss2 = T.batch_expected("snp65", int(acc.max()) + 1)
    assert np.array_equal(acc2, acc) and np.all(loss2 == 0)
    assert all(s.loss_ib > 0 for s in sc)
