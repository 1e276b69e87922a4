"""GPU parity of the batched scoring of a growth step (k_batch_cells + k_batch_scan, hibag_amd/csrc/hibag_build.hip) with the
oracle, at every SNP word count and on both of its routes, through hibag_hip_test_build_eval_batch.

The training driver reaches these kernels only through real greedy growth, which stops long before 33 SNPs, always keeps
the cohort on the device and never builds a list of more than 1,024 haplotypes; so only batch_cells<1>, staged, on the
device-resident route had ever run under a test.  The inputs are constructed (tests/training_reference.py) and their
properties -- few degenerate samples, a top word that decides something, every raw missing code -- are checked on the
CPU for each case used here (tests/test_training_inputs_host.py).

Expected values per candidate c, all from the oracle, all compared exactly: the genotype is the base with SNP n_snp - 1
set from columns[c] (TGenotype::_SetSNP); acc_oob[c] = sum over the out-of-bag samples of Compare(_BestGuess, truth);
loss_ib[c] = -2 * sum over the in-bag samples of count * log(_PostProb) where acc_oob[c] reaches the running maximum that
starts at acc_floor (src/LibHLA.cpp:2033-2034), else exactly 0.

The entry replaces the process's build state: nothing else runs between its init and its done, and no trainer runs
beside these tests.
"""

import ctypes as C

import numpy as np
import pytest

import training_reference as T

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_batch(b, acc_floor, device_route):
    """One call of the test entry.  device_route: the candidates' columns travel as rows of a SNP-major matrix that is
    kept on the device (`gdev` / derived ranges / `true_pair` in the kernels) -- and `columns` is NOT given, so a result
    can only come from the matrix; otherwise the host packs them (`cand_w` / `cellb` / `wpos`)."""
    import hibag_amd
    from hibag_amd import _lib
    hibag_amd.hlaSetKernelTarget("hip")
    n_cand, n = b.columns.shape
    boot = np.ascontiguousarray(b.boot, np.int32)
    geno = b.records()
    hap = np.concatenate([l.records() for l in b.lists])
    n_haplo = np.array([len(l.allele) for l in b.lists], np.int32)
    columns = np.ascontiguousarray(b.columns, np.int32)
    acc = np.full(n_cand, -7, np.int32)
    loss = np.full(n_cand, -7.0)
    if device_route:
        # the matrix holds other rows too, and the candidates' rows in another order than the candidates
        decoy = np.full((1, n), 2, np.int32)
        matrix = np.ascontiguousarray(np.concatenate([decoy, columns[::-1], decoy]))
        cand_snp = np.array([n_cand - c for c in range(n_cand)], np.int32)
        args = (None, _ptr(matrix), len(matrix), _ptr(cand_snp))
    else:
        args = (_ptr(columns), None, 0, None)
    _lib.check(_lib.lib().hibag_hip_test_build_eval_batch(
        b.n_hla, n, _ptr(boot), _ptr(geno), b.n_snp, n_cand, _ptr(n_haplo), _ptr(hap), *args, int(acc_floor), _ptr(acc), _ptr(loss)))
    return acc, loss


def check(key, acc_floor=0, routes=(True, False)):
    b = T.batch_case(key)
    want_acc, want_loss = T.batch_expected(key, acc_floor)
    got = [run_batch(b, acc_floor, r) for r in routes]
    for r, (acc, loss) in zip(routes, got):
        print(f"{key} floor {acc_floor} {'device-resident' if r else 'host-packed'}: acc {acc.tolist()} want {want_acc.tolist()}; "
              f"loss {loss.tolist()} want {want_loss.tolist()}")
    for r, (acc, loss) in zip(routes, got):
        route = "device-resident" if r else "host-packed"
        assert np.array_equal(acc, want_acc), route
        assert np.array_equal(loss, want_loss), route
    for acc, loss in got[1:]:                       # (follows from the above; stated because it is the routes' contract)
        assert np.array_equal(acc, got[0][0]) and np.array_equal(loss, got[0][1])
    return want_acc, want_loss


@pytest.mark.parametrize("n_snp", T.BATCH_WIDTHS)
def test_every_word_count_on_both_routes(n_snp, oracle):
    """3 candidates x 65 samples (two sample groups, the second a single lane) at n_snp = 1, 32 | 33, 64 | 65, 96 | 97, 128:
    batch_cells<1> | <2> | <3> | <4>, staged, with the candidate SNP at bit 0 and at bit 31 of each word
    (word = (n_snp - 1) >> 5, bit = (n_snp - 1) & 31).  Each once with the matrix (`gdev`, ranges derived from `cells` and
    `start`, `true_pair` compared in the scan) and once without (`cand_w`, `cellb`, `wpos`): the host-packed route first
    runs under a test here, at any width."""
    check(f"snp{n_snp}")


@pytest.mark.parametrize("p", T.CELL_ALLELES)
def test_cell_lists_around_the_scan_groups(p, oracle):
    """p = 2, 7, 8, 11, 63 present alleles -> 3, 28, 36, 66, 2,016 cells against k_batch_scan's groups of SCAN_NB = 32 that
    take turns in two buffers: less than one group; one group (padded); into the second group; past two groups (the first
    buffer's second turn); 63 full groups, an odd number and no padding.  64 samples x 2 candidates -> 64 segments: for
    p = 2 more segments than cells, so most segments are empty.  n_snp = 40: batch_cells<2>."""
    b = T.batch_case(f"cells-p{p}")
    assert [int(np.sum(l.lens > 0)) for l in b.lists] == [p, p]
    check(f"cells-p{p}")


def test_more_cells_than_segments(oracle):
    """256 samples (four sample groups: one workgroup of k_batch_cells holds all four) x 18 candidates -> 64 segments
    against 210 cells (p = 20): segments of several cells, cut by work."""
    check("cells-p20-n256")


def test_direct_and_staged_workgroups_in_one_launch(oracle):
    """Candidate 0 has 1,100 haplotypes over 4 alleles -- more than BATCH_LDS_HAPLO = 1,024, so its workgroups read the
    list from global memory (batch_cells<4>, direct) --, candidate 1 has 40 (staged in LDS, its list starting at haplotype
    1,100 of the launch's arrays): both kinds of workgroup in one launch, n_snp = 97, 64 samples."""
    b = T.batch_case("direct")
    assert [len(l.allele) for l in b.lists] == [1100, 40]
    check("direct")


def test_floor_rule(oracle):
    """acc_floor above every candidate's count: every loss is exactly 0 and the counts are still right.  acc_floor = 0:
    the first candidate's loss is computed, a later one's where its count reaches the running maximum."""
    acc, loss = check("snp65", acc_floor=0)
    assert loss[0] != 0
    top = int(acc.max()) + 1
    acc2, loss2 = check("snp65", acc_floor=top)
    assert np.array_equal(acc2, acc) and np.all(loss2 == 0)
    # a floor between the counts: candidates below it get no loss
    mid = int(acc.max())
    acc3, loss3 = check("snp65", acc_floor=mid, routes=(True,))
    assert [l != 0 for l in loss3] == [a >= mid for a in acc3]


def test_far_sample(oracle):
    """One sample is far from every haplotype pair: its cells are all 0, it has no best guess (which counts as no
    correct allele) and its posterior is 0 / 0 = NaN.  It is kept OUT-OF-BAG, so that loss_ib stays finite and compares
    with ==; an in-bag one would make the loss NaN on both sides."""
    b = T.batch_case("far")
    assert b.far >= 0 and b.boot[b.far] == 0
    acc, loss = check("far")
    assert np.all(np.isfinite(loss))
