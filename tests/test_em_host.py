"""CPU checks behind tests/test_hip_em.py: the Python reference of the EM fit (tests/em_reference.py) equals the oracle's
trainer bit for bit on every constructed case, every case that is compared on the device is DECIDED (its stopping test
stays more than 4 x the kernel's slack away from the tolerance at every iteration, so the kernel may not hand it back),
the cases have the shapes they are there for, and the fit's test entry refuses every bad argument without a device."""

import ctypes as C
import math

import numpy as np
import pytest

import em_reference as R

CASES = list(R.case_table())
GATHER_CASES = {"lists_gather", "haps4000"}
HAND_BACK = {"hb_empty", "hb_incompatible"}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_the_oracle(name, oracle):
    """em_reference.fit against oracle_em_fit (the oracle's own expectation_maximization on the same pair lists and
    flags): frequencies as bits, and the iteration count."""
    c = R.case(name)
    for k, (freq, iters, _) in enumerate(R.reference(name)):
        want, want_iters = oracle.em_fit(c.h1, c.h2, c.off, c.boot, c.geno[k].astype(np.int32), c.cur_freq, float(c.afreq[k]),
                                         c.n_samp_total)
        assert iters == want_iters, (name, k)
        assert np.array_equal(_bits(freq), _bits(want)), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_every_compared_fit_is_decided(name):
    """Margin of the stopping test over the kernel's slack, per candidate: above 4 at every iteration wherever the
    device's result is compared.  The two hand-back cases are the exception: their first log-likelihood is -inf."""
    ref = R.reference(name)
    low = [min(d["margin"]) for _, _, d in ref]
    print(f"{name}: iterations {[it for _, it, _ in ref]}, smallest margin / slack {['%.3g' % m for m in low]}")
    if name in HAND_BACK:
        assert R.case(name).hand_back
        for _, _, d in ref:
            assert d["loglik"][0] == -math.inf and not d["decided"]
        return
    assert not R.case(name).hand_back
    for k, (_, _, d) in enumerate(ref):
        assert math.isfinite(d["loglik"][0]), (name, k)
        assert d["decided"] and min(d["margin"]) > R.DECIDED_FACTOR, (name, k, min(d["margin"]))


def test_layouts_of_the_table():
    """The layout every case gets from the library's own rule (hibag_hip_test_em_layout: what hibag_em_fit_batch uses), and
    that rule against its restatement (em_reference.expected_layout) across both of its thresholds."""
    from hibag_amd import _lib
    L = _lib.lib()
    seen = set()
    for name in CASES:
        c = R.case(name)
        want = R.GATHER if name in GATHER_CASES else R.STAGED
        assert L.hibag_hip_test_em_layout(c.n_ib, c.n_pair, c.n_hap) == want == c.layout, name
        seen.add(want)
    assert seen == {R.STAGED, R.GATHER}
    # just past the largest cases: more haplotypes than haps4000 until nothing fits, more pairs than pairs4101 until the
    # lists' own copy of G no longer does
    c = R.case("haps4000")
    assert R.lds_bytes(c.n_ib, c.n_pair, c.n_hap, False) > 150 * 1024
    got = [L.hibag_hip_test_em_layout(c.n_ib, c.n_pair, nh) for nh in range(c.n_hap, c.n_hap + 400, 2)]
    assert got == [R.expected_layout(c.n_ib, c.n_pair, nh) for nh in range(c.n_hap, c.n_hap + 400, 2)]
    assert got[0] == R.GATHER and got[-1] == 0 and sorted(got, reverse=True) == got
    assert L.hibag_hip_test_em_layout(c.n_ib, c.n_pair, 4162) == R.GATHER and L.hibag_hip_test_em_layout(c.n_ib, c.n_pair, 4164) == 0
    c = R.case("pairs4101")
    assert R.lds_bytes(c.n_ib, c.n_pair, c.n_hap, True) > 144 * 1024
    got = [L.hibag_hip_test_em_layout(c.n_ib, n, c.n_hap) for n in range(c.n_pair, c.n_pair + 600)]
    assert got == [R.expected_layout(c.n_ib, n, c.n_hap) for n in range(c.n_pair, c.n_pair + 600)]
    assert got[0] == R.STAGED and got[-1] == R.GATHER and sorted(got) == got
    # the limits that are no matter of LDS
    for dims in ((0, 10, 4), (65536, 10, 4), (10, 65536, 4), (10, 10, 16386), (-1, 10, 4), (10, -1, 4), (10, 10, -2)):
        assert L.hibag_hip_test_em_layout(*dims) == 0, dims


def test_shapes_of_the_table():
    """What each case is there for."""
    for n in R.SAMPLE_COUNTS:
        c = R.case(f"n{n}")
        assert c.n_ib == n and c.n_cand == 4
    assert set(R.case("psum").pairs_per_sample()) == set(R.PAIRS_PER_SAMPLE)
    c = R.case("lists_staged")
    assert set(c.list_lengths()) == set(R.LIST_LENGTHS)
    assert int(np.sum(c.h1 == c.h2)) >= 10
    c = R.case("lists_gather")
    assert set(R.LIST_LENGTHS) <= set(c.list_lengths()) and (c.n_pair, c.n_ib, c.n_hap) == (5001, 300, 60)
    assert int(np.sum(c.h1 == c.h2)) >= 10
    c = R.case("pairs4101")
    assert (c.n_pair, c.n_ib, c.n_hap) == (4101, 200, 40) and c.n_pair % 4 and c.n_pair > 4 * 960
    assert R.case("pairs1003").n_pair == 1003
    c = R.case("samples1000")
    assert c.n_ib == 1000 and 2900 <= c.n_pair <= 3100
    c = R.case("haps4000")
    assert (c.n_hap, c.n_pair, c.n_ib) == (4000, 300, 100)
    assert max(c.h1.max(), c.h2.max()) == 3999 and int(np.sum(c.list_lengths() == 0)) > 3000
    assert int(np.sum(np.maximum(c.h1, c.h2) > 2048)) > 50
    assert [R.case(f"cand{n}").n_cand for n in (1, 8, 40)] == [1, 8, 40]
    c = R.case("hb_empty")
    assert 0 in c.pairs_per_sample()
    c = R.case("hb_incompatible")
    i = 6
    sums = {(int(a) & 1) + (int(b) & 1) for a, b in zip(c.h1[c.off[i]:c.off[i + 1]], c.h2[c.off[i]:c.off[i + 1]])}
    assert sums == {0} and np.all(c.geno[:, i] == 2)
    for name in CASES:
        c = R.case(name)
        assert c.boot.min() >= 1 and c.boot.max() <= 9 and c.n_samp_total > c.n_ib
        assert c.off[0] == 0 and c.off[-1] == c.n_pair == len(c.h1) == len(c.h2) and c.n_hap == 2 * len(c.cur_freq)
        assert min(c.h1.min(), c.h2.min()) >= 0 and max(c.h1.max(), c.h2.max()) < c.n_hap
        assert set(np.unique(c.geno)) <= {0, 1, 2, 3} and c.geno.dtype == np.int8 and c.geno.shape == (c.n_cand, c.n_ib)
        all_missing = [k for k in range(c.n_cand) if np.all(c.geno[k] == 3)]
        assert len(all_missing) == (0 if name == "hb_incompatible" else 1), name
        for k in range(c.n_cand):
            assert 0 < c.afreq[k] < 1
            if k not in all_missing:
                assert c.afreq[k] == R.afreq_in_bag(c.geno[k], c.boot), (name, k)         # as prepare_new_snp computes it
    typed = np.concatenate([R.case(n).geno[:-1].ravel() for n in CASES if n not in HAND_BACK and R.case(n).n_cand > 1
                            and n not in R.SPEED_CASES and n not in R.UNDERFLOW_CASES])
    assert 0.03 < np.mean(typed == 3) < 0.07                                   # about 5 % missing


def test_iteration_counts_of_the_table():
    """Fast and slow fits at both parities of the count, the 500-iteration cap, and the table's extremes."""
    its = {name: [it for _, it, _ in R.reference(name)] for name in CASES if name not in HAND_BACK}
    for name, want in R.SPEED_ITERS.items():
        assert its[name][0] == want, name
    assert R.SPEED_ITERS["fast_even"] <= 20 and R.SPEED_ITERS["fast_odd"] <= 20 and R.SPEED_ITERS["fast_even"] % 2 == 0
    assert R.SPEED_ITERS["slow_even"] >= 200 and R.SPEED_ITERS["slow_odd"] >= 200 and R.SPEED_ITERS["slow_odd"] % 2 == 1
    assert R.SPEED_ITERS["capped"] == R.EM_MAX_ITER + 1
    flat = [v for l in its.values() for v in l]
    assert (min(flat), max(flat)) == (2, 501)
    assert its["pairs4101"][-1] == 501 and its["pairs1003"][-1] == 501          # the cap in a large step too


def test_underflow_cases_tell_the_order_of_the_doubling():
    """2 * f1 * f2 left to right and 2 * (f1 * f2) are the same number until f1 * f2 is subnormal.  The underflow cases end with
    a haplotype's frequency down there, and the reference with the doubling moved gives other bits on each of them (and the
    same bits on a case that stays in the normal range) -- so a kernel that doubles late fails on them and only there."""
    import sys
    for name in R.UNDERFLOW_CASES:
        c = R.case(name)
        freq, iters, _ = R.reference(name)[0]
        assert np.any((freq > 0) & (freq < sys.float_info.min)), name
        other, other_iters, _ = R.fit(c.h1, c.h2, c.off, c.boot, c.geno[0], c.cur_freq, float(c.afreq[0]), c.n_samp_total, two_last=True)
        assert other_iters == iters and not np.array_equal(_bits(other), _bits(freq)), name
    c = R.case("n9")
    freq, iters, _ = R.reference("n9")[0]
    other, other_iters, _ = R.fit(c.h1, c.h2, c.off, c.boot, c.geno[0], c.cur_freq, float(c.afreq[0]), c.n_samp_total, two_last=True)
    assert other_iters == iters and np.array_equal(_bits(other), _bits(freq))


def test_em_fit_entry_rejects_bad_arguments_without_a_gpu():
    """hibag_hip_test_em_fit checks everything the kernel indexes with before it touches the device: every bad call
    answers HIBAG_HIP_EINVAL with a message, with or without a device."""
    from hibag_amd import _lib
    L = _lib.lib()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_ib, n_pair, n_hap, n_cand = 2, 3, 4, 2

    def arrays():
        return dict(h1=i32([0, 1, 2]), h2=i32([1, 3, 2]), off=i32([0, 2, 3]), boot=i32([1, 2]), cur=np.array([0.4, 0.6]),
                    geno=np.array([[0, 1], [3, 2]], np.int8), af=np.array([0.25, 0.5]), out=np.zeros((n_cand, n_hap)),
                    status=i32([0, 0]), iters=i32([0, 0]), layout=i32([0]))

    def call(sizes=(n_ib, n_pair, n_hap, 5), n_c=n_cand, null=None, **change):
        a = arrays()
        for k, (at, v) in change.items():
            a[k].reshape(-1)[at] = v
        ptr = {k: (None if k == null else p(v)) for k, v in a.items()}
        rc = L.hibag_hip_test_em_fit(*sizes, ptr["h1"], ptr["h2"], ptr["off"], ptr["boot"], ptr["cur"], n_c, ptr["geno"], ptr["af"],
                                     ptr["out"], ptr["status"], ptr["iters"], ptr["layout"])
        return rc, L.hibag_hip_last_error().decode()

    bad = [dict(sizes=(0, n_pair, n_hap, 5)), dict(sizes=(n_ib, 0, n_hap, 5)), dict(sizes=(n_ib, n_pair, 0, 5)),
           dict(sizes=(n_ib, n_pair, n_hap, 0)), dict(sizes=(-1, n_pair, n_hap, 5)), dict(n_c=0), dict(n_c=-3),
           dict(sizes=(n_ib, n_pair, 5, 5)),                                                    # odd n_hap
           dict(sizes=(n_ib, n_pair, 20000, 5)), dict(sizes=(70000, n_pair, n_hap, 5)),         # hibag_em_fits() false
           dict(off=(0, 1)), dict(off=(0, -1)), dict(off=(1, 4)), dict(off=(2, 2)), dict(off=(2, 4)),
           dict(h1=(0, -1)), dict(h1=(2, n_hap)), dict(h2=(1, -1)), dict(h2=(0, n_hap)), dict(h2=(2, 1 << 20)),
           dict(boot=(0, 0)), dict(boot=(1, -2)),
           dict(geno=(0, 4)), dict(geno=(3, -1)), dict(geno=(1, 127)),
           dict(af=(0, 0.0)), dict(af=(1, 1.0)), dict(af=(0, -0.5)), dict(af=(1, 1.5)), dict(af=(0, math.nan))]
    bad += [dict(null=k) for k in ("h1", "h2", "off", "boot", "cur", "geno", "af", "out", "status")]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and "test_em_fit" in msg, (kw, rc, msg)
    assert "does not fit" in call(sizes=(n_ib, n_pair, 20000, 5))[1]
    assert "odd" in call(sizes=(n_ib, n_pair, 5, 5))[1]
    assert "outside" in call(h2=(0, n_hap))[1]
    tr = L.hibag_hip_trainer_em_counts(None, None)
    assert tr == -1
