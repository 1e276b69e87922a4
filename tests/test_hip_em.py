"""GPU parity of the device EM fit (k_em_fit, hibag_amd/csrc/hibag_em.hip) with the reference's EM, one growth step at a
time through hibag_hip_test_em_fit.

The training driver shows only the winner of every growth step, fits silently on the host whatever the kernel hands back,
and reaches the kernel's two LDS layouts and the edges of its unrolled loops by accident of a step's size.  Here every
candidate of every constructed step (tests/em_reference.py) is compared with a plain Python restatement of
CAlg_EM::ExpectationMaximization (src/LibHLA.cpp:1185-1255) that tests/test_em_host.py holds to the oracle's trainer bit
for bit: status 1, the same iteration count, and the frequencies equal AS BITS.

The kernel may answer 2 ("the host must fit it") only where its stopping test comes within its documented slack of the
tolerance.  Every compared candidate keeps more than 4 x that slack at every iteration (asserted on the CPU), so the cap on
hand-backs here is zero; the two hand-back cases, whose first log-likelihood is -inf, must answer 2 for every candidate.
The `layout` output says which LDS layout really ran: shapes select it, and both run here.
"""

import ctypes as C

import numpy as np
import pytest

import em_reference as R

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_fit(c):
    """One call of the test entry on a case: (out_freq [n_cand][n_hap], status, iters, layout)."""
    import hibag_amd
    from hibag_amd import _lib
    hibag_amd.hlaSetKernelTarget("hip")
    out = np.full((c.n_cand, c.n_hap), np.nan)
    status = np.full(c.n_cand, -7, np.int32)
    iters = np.full(c.n_cand, -7, np.int32)
    layout = np.full(1, -7, np.int32)
    _lib.check(_lib.lib().hibag_hip_test_em_fit(
        c.n_ib, c.n_pair, c.n_hap, c.n_samp_total, _ptr(c.h1), _ptr(c.h2), _ptr(c.off), _ptr(c.boot), _ptr(c.cur_freq), c.n_cand,
        _ptr(c.geno), _ptr(c.afreq), _ptr(out), _ptr(status), _ptr(iters), _ptr(layout)))
    return out, status, iters, int(layout[0])


def check(name, layout=None):
    c = R.case(name)
    ref = R.reference(name)
    out, status, iters, ran = run_fit(c)
    want_iters = [it for _, it, _ in ref]
    same = [bool(np.array_equal(out[k].view(np.uint64), ref[k][0].view(np.uint64))) for k in range(c.n_cand)]
    print(f"{name}: {c.n_ib} samples, {c.n_pair} pairs, {c.n_hap} haplotypes, layout {ran}; status {status.tolist()}; "
          f"iterations {iters.tolist()} want {want_iters}; frequencies equal as bits {same}")
    assert ran == c.layout and (layout is None or ran == layout)
    if c.hand_back:
        # the kernel's defined answer to a log-likelihood of -inf; the frequencies are not compared
        assert all(d["loglik"][0] == -np.inf for _, _, d in ref)
        assert status.tolist() == [2] * c.n_cand
        return out, status, iters
    for k, (freq, it, d) in enumerate(ref):
        assert d["decided"], (name, k)                  # (fixed inputs: tests/test_em_host.py checks the same)
        assert status[k] == 1, (name, k)
        assert iters[k] == it, (name, k)
        assert np.array_equal(out[k].view(np.uint64), freq.view(np.uint64)), (name, k)
    return out, status, iters


@pytest.mark.parametrize("n_ib", R.SAMPLE_COUNTS)
def test_sample_counts(n_ib):
    """1 ... 257 samples, ~3 base pairs each, 4 candidates: the log-likelihood chain's four pieces and its eight-term
    pipelined groups empty, shorter than 8, exactly 8, 9-15, 16 and more; partial wavefronts in every phase."""
    check(f"n{n_ib}")


def test_pairs_per_sample():
    """Samples with 1, 3, 4, 15, 16, 17, 31, 32, 33, 48 pairs: psum's 16-wide groups and its tail."""
    check("psum")


def test_list_lengths_staged():
    """Haplotypes in 0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33 pair entries, homozygous pairs among them, in the
    staged layout: the lists' padding to 4, the 16- and 4-wide loops, the two neighbouring positions of (h, h); a
    haplotype in no pair gets 0 and then gives zero products."""
    check("lists_staged", R.STAGED)


def test_list_lengths_gather():
    """The same lengths inside 5,001 pairs of 300 samples on 60 haplotypes, where only the gather layout fits: the
    8-entry pipelined gather, both of its exits, the +0.0 slot behind G."""
    check("lists_gather", R.GATHER)


@pytest.mark.parametrize("n_pair", [4101, 1003])
def test_many_pairs(n_pair):
    """More pairs than four per worker thread (4,101: staged at ~148 KB of LDS) and a count that is no multiple of 4: a
    second turn of the pair phases, the clamped look-ups behind the last pair.  The all-missing candidate of both
    runs all 500 iterations."""
    check(f"pairs{n_pair}", R.STAGED)


def test_many_samples():
    """1,000 samples: a second turn of the sample phase, the term buffers at size."""
    check("samples1000")


def test_many_haplotypes():
    """4,000 doubled haplotypes (gather): several turns of the haplotype phase, most lists empty, indices past 2,048."""
    check("haps4000", R.GATHER)


@pytest.mark.parametrize("n_cand", [1, 8, 40])
def test_candidate_counts(n_cand):
    """1, 8, 40 workgroups on one pair set: genotypes, frequencies, status and iterations indexed by workgroup (the
    status array carries the iterations behind the statuses).  The same candidate gives the same bits in each."""
    out, _, iters = check(f"cand{n_cand}")
    if n_cand > 1:
        small = run_fit(R.case("cand1"))
        assert np.array_equal(small[0][0].view(np.uint64), out[-1].view(np.uint64)) and small[2][0] == iters[-1]


@pytest.mark.parametrize("name", list(R.SPEED_CASES))
def test_fast_and_slow_fits(name):
    """Fits that stop after 16 and 13 iterations, after 386 and 239, and one that never meets the stopping test: the
    verdict's one-iteration lag, the two frequency buffers at both parities, which of them is returned -- and the exit
    after 500 iterations, where it is the other one."""
    _, _, iters = check(name)
    assert iters[0] == R.SPEED_ITERS[name]


@pytest.mark.parametrize("name", list(R.UNDERFLOW_CASES))
def test_subnormal_frequencies(name):
    """Fits in which a haplotype's frequency decays into the subnormal range: FP64 subnormals in the products, the sums and
    the result, and the one place where doubling a heterozygous pair's product before or after the multiplication differs."""
    out, _, _ = check(name)
    assert np.any((out[0] > 0) & (out[0] < np.finfo(np.float64).tiny))


@pytest.mark.parametrize("name", ["hb_empty", "hb_incompatible"])
def test_hand_back(name):
    """A sample with no pair at all, and a sample none of whose pairs is compatible with its genotype: psum = 0, the
    log-likelihood is -inf, and the kernel's answer is status 2 for every candidate."""
    check(name)


def test_arena_reuse():
    """Small, largest, small again on one thread, and one case twice: the same bits every time."""
    first = check("n7")
    check("lists_gather")
    check("haps4000")
    again = check("n7")
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    a, b = check("lists_staged"), check("lists_staged")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
