"""Classifier-sharded prediction driven by the C library itself: hibag_hip_model_shard + hibag_hip_shard_group_* with the
posterior merge as ONE ncclAllReduce issued by libhibag_hip.so (hibag_amd/csrc/hibag_shard.hip).  The sum being split is
CAttrBag_Model::_PredictHLA's ensemble sum (src/LibHLA.cpp:2448-2476, :1497-1518); the reference's own multi-worker
branch is hlaPredict(cl=) (R/HIBAG.R:764-808).  Splitting the classifiers changes the order of their additions, so
against the UNSHARDED run the bar is identical calls and 1e-10 relative on the posteriors -- and bit equality where the
split is trivial (one shard).

Against the host restatement of the split itself (tests/shard_reference.py, pinned on the CPU by tests/test_shard_host.py)
the bar is the bits: a shard's partial sums [P + 3][n] are its classifiers' terms added in order from +0.0, shards that share
a device are added in shard order, a one-rank all-reduce is the identity, and the finish kernels are a pure function of the
merged sums -- fed here with planted sums at the edges a real prediction does not reach."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def hib():
    import hibag_amd
    hibag_amd.hlaSetKernelTarget("hip")
    return hibag_amd


@pytest.fixture(scope="module")
def case(hib):
    from hibag_amd import synth
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 3000)
    G[11, :] = hib.NA_INTEGER
    m = hib.hlaModelFromObj(model)
    full = m.predict_raw(G, 1, want_dosage=True, want_prob=True)
    return model, G, m, full


def close_to_unsharded(got, full):
    assert np.array_equal(got["h1"], full["h1"]) and np.array_equal(got["h2"], full["h2"])
    fin = np.isfinite(full["postprob"]).all(axis=1)
    assert np.array_equal(np.isnan(got["postprob"]), np.isnan(full["postprob"]))
    for k in ("prob", "matching", "dosage", "postprob"):
        np.testing.assert_allclose(got[k][fin], full[k][fin], rtol=TOL, atol=1e-300, err_msg=k)


def test_one_shard_one_rccl_rank_equals_the_unsharded_run_bit_for_bit(hib, case):
    """A 1-device communicator: the all-reduce is the identity, the partial + finish route must reproduce the plain entry."""
    from hibag_amd.hibag import ShardGroup
    model, G, m, full = case
    assert hib._lib.lib().hibag_hip_rccl_version() >= 20000
    grp = ShardGroup(m, [0])
    assert grp.ranks == 1
    got = grp.predict_raw(G, want_dosage=True, want_prob=True)
    assert grp.allreduces >= 1
    for k in ("h1", "h2", "prob", "matching", "dosage", "postprob"):
        assert np.array_equal(got[k], full[k], equal_nan=True), k
    for s in grp.shards:
        assert s.handover_faults() == 0
    grp.close()


@pytest.mark.parametrize("n_shards", [2, 8])
def test_shards_sharing_the_device_merge_like_ranks_would(hib, case, n_shards):
    """Several shards on the one device of the box: added up on the device in shard order, then the (1-rank) all-reduce."""
    from hibag_amd.hibag import ShardGroup
    model, G, m, full = case
    grp = ShardGroup(m, [0] * n_shards)
    assert grp.ranks == 1 and len(grp.shards) == n_shards
    counts = [hib._lib.lib().hibag_hip_model_n_classifier(s.handle) for s in grp.shards]
    assert sum(counts) == len(model.classifiers) and max(counts) - min(counts) <= 1
    got = grp.predict_raw(G, want_dosage=True, want_prob=True)
    close_to_unsharded(got, full)
    # only the calls
    only = grp.predict_raw(G[:100], want_dosage=False, want_prob=False)
    assert np.array_equal(only["h1"], full["h1"][:100]) and np.array_equal(only["h2"], full["h2"][:100])
    grp.close()


def test_one_shot_entry_and_errors(hib, case):
    model, G, m, full = case
    L = hib._lib.lib()
    s0, s1 = m.shard(0, 2, 0), m.shard(1, 2, 0)
    n = 500
    g = np.ascontiguousarray(G[:n], np.int32)
    h1 = np.zeros(n, np.int32); h2 = np.zeros(n, np.int32); pr = np.zeros(n); mt = np.zeros(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    hs = (C.c_void_p * 2)(s0.handle, s1.handle)
    hib._lib.check(L.hibag_hip_predict_multi_sharded(hs, 2, p(g), n, p(h1), p(h2), p(pr), p(mt), None, None))
    assert np.array_equal(h1, full["h1"][:n]) and np.array_equal(h2, full["h2"][:n])
    np.testing.assert_allclose(pr, full["prob"][:n], rtol=TOL)
    np.testing.assert_allclose(mt, full["matching"][:n], rtol=TOL)
    # H1 without H2, no shards
    assert L.hibag_hip_predict_multi_sharded(hs, 2, p(g), n, p(h1), None, None, None, None, None) != 0
    assert L.hibag_hip_predict_multi_sharded(hs, 0, p(g), n, p(h1), p(h2), None, None, None, None) != 0
    with pytest.raises(hib.HibagHipError):
        m.shard(0, 2, 99)
    with pytest.raises(hib.HibagHipError):
        m.shard(2, 2, 0)
    s0.close(); s1.close()


def test_a_failed_handover_on_one_shard_is_repaired_not_returned(hib):
    """The poisoned scalar rows of one shard reach the merged sums as NaN; the group entry must notice (sticky status of
    the shard), run the batch again without hand-overs, and return the repaired numbers."""
    from hibag_amd import synth
    from hibag_amd.hibag import ShardGroup
    model, founders, af = synth.make_model("hla-b")
    G, _ = synth.make_samples(founders, af, 10_000)
    m = hib.hlaModelFromObj(model)
    full = m.predict_raw(G, 1, want_dosage=True, want_prob=False)
    grp = ShardGroup(m, [0])                      # one shard = the whole model: its items are chunked at 10,000 samples
    grp.shards[0].inject_handover_fault(2)
    got = grp.predict_raw(G, want_dosage=True, want_prob=False)
    assert grp.shards[0].handover_faults() == 1 and grp.shards[0].status() == 0
    for k in ("h1", "h2", "prob", "matching", "dosage"):
        assert np.array_equal(got[k], full[k], equal_nan=True), k
    grp.close(); m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--no-cpu-baseline"], ["--shard", "classifiers"]])
def test_bench_two_rank_rehearsal_on_one_device(extra, tmp_path, oracle):
    """`python bench.py --gpus 2` end to end on a one-GPU box: bench.py starts its own two ranks (torch.distributed.run), both
    ranks share device 0 and the collectives go over gloo (HIBAG_BENCH_DRY_RANKS=1 -- RCCL refuses two ranks on one device).
    What is checked is the orchestration the driver's 8-GPU run goes through: slice bounds, the classifier-sharded merge
    against the unsharded posterior, the one JSON line -- and --dump-outputs: rank 0 writes every rank's share of the
    100,000 samples, which must be the oracle's outputs across the boundary between the ranks' slices."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HIBAG_BENCH_DRY_RANKS="1")
    dump = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--full", "--dump-outputs", dump] + extra,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["samples_per_step"] == 100_000
    assert "dry_run" in d and d["rccl_ranks"] is None
    assert d["call_accuracy_vs_truth"] > 0.99
    chk = d["classifier_shard_check"] if "--shard" in extra else d["classifier_sharded"]["check"]
    assert chk["calls_identical_to_unsharded"] and chk["nan_pattern_identical"]
    assert chk["max_rel_dev_posterior_vs_unsharded"] < chk["tolerance"]
    assert all(v == 0 for v in d["handover_faults"].values())
    import bench
    from hibag_amd import synth
    got = bench.read_dump(dump)
    assert np.array_equal(got.pop("sample_index"), np.arange(100_000))
    model, founders, af = synth.make_model(bench.SHAPE)
    geno, _ = synth.make_samples(founders, af, 100_000, seed=synth.DEFAULT_SEED + 1)
    rows = np.r_[0:500, 49_000:51_000, 99_500:100_000]
    want = oracle.predict(oracle.flatten(model), geno[rows], vote_method=1, avx2=True, n_threads=8)
    for k, v in got.items():
        w = np.asarray(want[k], np.float64)
        if "--shard" in extra and k not in ("h1", "h2"):      # (the merged partial sums: rounding-level differences)
            assert np.array_equal(np.isnan(v[rows]), np.isnan(w)), k
            fin = np.isfinite(w) & (np.abs(w) > 1e-200)
            np.testing.assert_allclose(v[rows][fin], w[fin], rtol=chk["tolerance"], atol=0, err_msg=k)
        else:
            assert np.array_equal(v[rows], w, equal_nan=True), k


# ---- the bits: partial sums, merge and finish against tests/shard_reference.py ----------------------------------------

def _bounds(hib, n_classifier, world, r):
    first, count = C.c_int(-1), C.c_int(-1)
    hib._lib.check(hib._lib.lib().hibag_hip_shard_bounds(n_classifier, world, r, C.byref(first), C.byref(count)))
    return first.value, first.value + count.value


def _partial_on_device(shard, G):
    """hibag_hip_predict_partial_device of one shard: float64 [P + 3, n] (the padding columns are dropped)."""
    import torch
    dev = torch.device("cuda", 0)
    n, P = G.shape[0], shard.obj.n_cell
    g = torch.from_numpy(np.ascontiguousarray(G, np.int32)).to(dev)
    part = torch.full((P + 3, (n + 63) // 64 * 64), -7.0, dtype=torch.float64, device=dev)       # (every real column must be written)
    shard.predict_partial_device(g.data_ptr(), n, part.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert shard.status() == 0
    return part.cpu().numpy()[:, :n]


FINISH_SETS = (("h1", "h2", "prob", "matching"), ("h1", "h2", "prob", "matching", "dosage"),
               ("h1", "h2", "prob", "matching", "dosage", "postprob"))          # k_finish_call; k_finish; k_finish + k_finish_prob


def _finish_on_device(m, sums, n, keys):
    """hibag_hip_finish_device on the merged sums float64 [P + 3, n_pad] for the outputs `keys`."""
    import torch
    dev = torch.device("cuda", 0)
    P, n_hla = m.obj.n_cell, m.obj.n_hla
    assert sums.shape == (P + 3, (n + 63) // 64 * 64) and sums.dtype == np.float64
    d = torch.from_numpy(np.ascontiguousarray(sums)).to(dev)
    shape = dict(h1=(n,), h2=(n,), prob=(n,), matching=(n,), dosage=(n, n_hla), postprob=(n, P))
    out = {k: (torch.full(shape[k], -77, dtype=torch.int32, device=dev) if k in ("h1", "h2") else
               torch.full(shape[k], -7.0, dtype=torch.float64, device=dev)) for k in keys}
    ptr = lambda k: out[k].data_ptr() if k in out else None
    m.finish_device(d.data_ptr(), n, ptr("h1"), ptr("h2"), ptr("prob"), ptr("matching"), ptr("dosage"), ptr("postprob"),
                    stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


WORLDS = (1, 2, 3, 5, 13)


@pytest.fixture(scope="module")
def hand(hib, oracle):
    """The hand-built 13-classifier model and its 130 samples (shard_reference.hand_model / hand_samples), the restatement's
    partial sums of every shard of every split -- computed once, never changed -- and the oracle's outputs."""
    import shard_reference as R
    model, founders = R.hand_model()
    G = R.hand_samples(model, founders)
    fm = oracle.flatten(model)
    parts = {w: R.shard_parts(oracle, fm, model, w, G) for w in WORLDS}
    for ps in parts.values():
        for p_ in ps:
            p_.setflags(write=False)
    want = oracle.predict(fm, G, vote_method=1)
    m = hib.hlaModelFromObj(model)
    yield model, G, m, parts, want
    m.close()


def test_the_hand_built_case_reaches_every_engine_and_skips_classifiers(hib, hand):
    import shard_reference as R
    model, G, m, parts, want = hand
    assert model.n_hla == 5 and model.n_cell == 15 == R.FIN_SEG - 1 and len(model.classifiers) == 13 and G.shape == (130, 142)
    eng = [m.engine(c) for c in range(13) if c != R.HAND_EMPTY_AT]
    assert [len(model.classifiers[c].snpidx) for c in range(13) if c != R.HAND_EMPTY_AT] == list(R.HAND_WIDTHS)
    names, steps = [e for e, k in eng], [k for e, k in eng]
    assert names[:4] == ["fp4"] * 4 and steps[:4] == [1] * 4                           # 3, 14, 28, 29: FP4 in one K step
    assert names[4:6] == ["i8"] * 2                                                    # 31, 32: int8
    assert names[6:10] == ["fp4"] * 4 and min(steps[6:10]) >= 2                        # 33, 60, 100, 112: FP4 in several
    assert names[10:] == ["valu"] * 2                                                  # 113, 128
    W = R.classifier_weights(model, G)
    assert (W[list(R.HAND_SKIPPED), 64:67] == 0).all() and (W[R.HAND_GROUP_SKIPPED, 64:128] == 0).all() and (W[:, 5] == 0).all()
    assert (W[:, 64] > 0).sum() >= 8 and np.flatnonzero(W[R.HAND_EMPTY_AT] > 0).tolist() == sorted(R.HAND_USE_EMPTY)
    # in the 2-, 3- and 5-shard splits the skipped classifiers sit in shards with others that are used
    for w in (2, 3, 5):
        for c in R.HAND_SKIPPED + (R.HAND_GROUP_SKIPPED,):
            lo, hi = next(_bounds(hib, 13, w, r) for r in range(w) if _bounds(hib, 13, w, r)[0] <= c < _bounds(hib, 13, w, r)[1])
            assert hi - lo >= 2 and (W[lo:hi, 64] > 0).any()
    for w in WORLDS:
        assert [_bounds(hib, 13, w, r) for r in range(w)] == [R.shard_bounds(13, w, r) for r in range(w)]


@pytest.mark.parametrize("world", WORLDS)
def test_partial_sums_of_every_shard_equal_the_restatement_bit_for_bit(hib, hand, world):
    """(3a) every row of [P + 3][n], cells and the three scalar rows, of every shard; again at n = 64 and n = 1."""
    import shard_reference as R
    model, G, m, parts, want = hand
    for r in range(world):
        shard = m.shard(r, world, 0)
        lo, hi = _bounds(hib, 13, world, r)
        assert hib._lib.lib().hibag_hip_model_n_classifier(shard.handle) == hi - lo
        for n in (130, 64, 1):
            got = _partial_on_device(shard, G[:n])
            R.assert_same_rows(got, parts[world][r][:, :n], what=f"shard {r} of {world} (classifiers {lo}..{hi - 1}), n = {n}:")
        assert shard.handover_faults() == 0
        shard.close()


@pytest.mark.parametrize("k", [2, 3, 5, 13])
def test_shard_group_on_one_device_equals_the_in_order_merge_bit_for_bit(hib, hand, k):
    """(3b) shards sharing the device are added in shard order, the one-rank all-reduce is the identity."""
    import shard_reference as R
    from hibag_amd.hibag import ShardGroup
    model, G, m, parts, want = hand
    ref = R.finish(R.merge(parts[k]), 5, 130)
    grp = ShardGroup(m, [0] * k)
    assert grp.ranks == 1 and len(grp.shards) == k
    got = grp.predict_raw(G, want_dosage=True, want_prob=True)
    R.assert_same(got, ref, what=f"{k} shards")
    five = grp.predict_raw(G, want_dosage=True, want_prob=False)
    assert "postprob" not in five
    R.assert_same(five, ref, keys=R.KEYS[:5], what=f"{k} shards, no posterior matrix")
    if k == 13:                                   # one classifier per shard: 0 + term is exact, the oracle's own order
        R.assert_same(got, want, what="13 shards against the oracle")
    for s in grp.shards:
        assert s.handover_faults() == 0 and s.status() == 0
    grp.close()


@pytest.mark.parametrize("want_prob", [True, False])
def test_one_shot_sharded_entry_equals_the_in_order_merge_bit_for_bit(hib, hand, want_prob):
    """(3b) hibag_hip_predict_multi_sharded with 3 shards."""
    import shard_reference as R
    model, G, m, parts, want = hand
    ref = R.finish(R.merge(parts[3]), 5, 130)
    shards = [m.shard(r, 3, 0) for r in range(3)]
    n = 130
    g = np.ascontiguousarray(G, np.int32)
    out = dict(h1=np.zeros(n, np.int32), h2=np.zeros(n, np.int32), prob=np.zeros(n), matching=np.zeros(n), dosage=np.zeros((n, 5)))
    if want_prob:
        out["postprob"] = np.zeros((n, 15))
    p = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
    hs = (C.c_void_p * 3)(*[s.handle for s in shards])
    hib._lib.check(hib._lib.lib().hibag_hip_predict_multi_sharded(hs, 3, g.ctypes.data_as(C.c_void_p), n, p("h1"), p("h2"), p("prob"),
                                                                 p("matching"), p("dosage"), p("postprob")))
    R.assert_same(out, ref, keys=R.KEYS if want_prob else R.KEYS[:5], what="one-shot entry, 3 shards")
    for s in shards:
        assert s.handover_faults() == 0
        s.close()


@pytest.fixture(scope="module")
def finish_models(hib):
    """A finalized model per allele count: hibag_hip_finish_device reads the model's n_hla and nothing else of it."""
    made = {}

    def get(n_hla):
        if n_hla not in made:
            obj = hib.HlaAttrBagObj(n_samp=0, n_snp=1, hla_allele=[f"{a:02d}" for a in range(n_hla)],
                                    classifiers=[hib.Classifier(snpidx=[0], freq=[1.0], hla=[0], haplo=["0"])])
            made[n_hla] = hib.hlaModelFromObj(obj)
        return made[n_hla]
    yield get
    for m in made.values():
        m.close()


def _check_finish(m, sums, n, what):
    import shard_reference as R
    ref = R.finish(sums, m.obj.n_hla, n)
    first = None
    for keys in FINISH_SETS:
        got = _finish_on_device(m, sums, n, keys)
        R.assert_same(got, ref, keys=keys, what=f"{what}, outputs {'+'.join(keys[3:])}:")
        if first is None:
            first = got
        R.assert_same(got, first, keys=FINISH_SETS[0], what=f"{what}, {'+'.join(keys[3:])} against the call-only launch:")


@pytest.mark.parametrize("n_hla", [1, 2, 5, 6, 16, 17, 23])
def test_finish_device_on_planted_sums_equals_the_host_finish_bit_for_bit(hib, finish_models, n_hla):
    """(3c) P = 1, 3, 15, 21, 136, 153, 276 cells against FIN_SEG = 16 segments of ceil(P / 16) cells and their eight-wide
    loops, n = 1, 64, 130; the planted columns (ties in a block, across blocks, across segments, after scaling; zero, NaN and
    subnormal weight sums; NaN, infinite and subnormal cells) are described and asserted in tests/test_shard_host.py.  Three
    output sets: k_finish_call alone, k_finish (call + dosage), k_finish + k_finish_prob."""
    import shard_reference as R
    m = finish_models(n_hla)
    assert m.obj.n_cell == n_hla * (n_hla + 1) // 2
    for n in (64, 130):
        sums, where = R.synthetic_merged(n_hla, n)
        assert {where[s] for s in where} == set(R.planted_sums(n_hla)[1])
        _check_finish(m, sums, n, f"n_hla {n_hla}, n {n}")
    planted, names = R.planted_sums(n_hla)
    for j, name in enumerate(names):              # n = 1: one planted column at a time
        sums = np.zeros((planted.shape[0], 64))
        sums[:, 0] = planted[:, j]
        sums[:, 1:] = R.synthetic_merged(n_hla, 64)[0][:, 1:]     # (what the padding lanes read: anything)
        _check_finish(m, sums, 1, f"n_hla {n_hla}, n 1, {name}")


def test_more_shards_than_classifiers_the_empty_shard_adds_zeros(hib, oracle):
    """(3d) 3 classifiers in 4 shards: hibag_hip_shard_bounds gives the last shard no classifier.  Its partial sums are all
    +0.0 -- cells and scalar rows -- and the group's result is the restatement's with that shard in the merge."""
    import shard_reference as R
    from hibag_amd.hibag import ShardGroup
    model, founders = R.hand_model(seed=77, widths=(7, 31, 40), empty_at=None)
    G = R.hand_samples(model, founders, 130, seed=78, structured=False)
    G[9, :] = hib.NA_INTEGER
    fm = oracle.flatten(model)
    assert [_bounds(hib, 3, 4, r) for r in range(4)] == [(0, 1), (1, 2), (2, 3), (3, 3)]
    parts = [R.partial_sums(oracle, fm, model, *R.shard_bounds(3, 4, r), G) for r in range(4)]
    assert parts[3].shape == (18, 192) and not parts[3].any() and not np.signbit(parts[3]).any()
    ref = R.finish(R.merge(parts), 5, 130)
    m = hib.hlaModelFromObj(model)
    empty = m.shard(3, 4, 0)
    assert hib._lib.lib().hibag_hip_model_n_classifier(empty.handle) == 0 and empty.batch_limit() >= 64
    for n in (130, 1):
        R.assert_same_rows(_partial_on_device(empty, G[:n]), parts[3][:, :n], what=f"the empty shard, n = {n}:")
    empty.close()
    grp = ShardGroup(m, [0] * 4)
    got = grp.predict_raw(G, want_dosage=True, want_prob=True)
    R.assert_same(got, ref, what="3 classifiers in 4 shards")
    R.assert_same(got, oracle.predict(fm, G, vote_method=1), what="3 classifiers in 4 shards against the oracle")
    for s in grp.shards:
        assert s.handover_faults() == 0 and s.status() == 0
    grp.close(); m.close()


def test_the_groups_batch_cut_is_invisible_in_the_bits(hib, oracle):
    """(3e) more samples than one batch of the group: the second batch starts at the cut, its outputs land behind the
    first's.  One classifier per shard, so every sample must be the oracle's in its bits."""
    import shard_reference as R
    from hibag_amd.hibag import ShardGroup
    model, founders = R.hand_model(seed=91, widths=(5, 9, 14, 20), empty_at=None)
    m = hib.hlaModelFromObj(model)
    grp = ShardGroup(m, [0] * 4)
    cut = min(min(s.batch_limit() for s in grp.shards), 32768) // 64 * 64
    assert cut >= 64
    n = cut + 70
    G = R.hand_samples(model, founders, n, seed=92, structured=False)
    G[cut - 1, :] = hib.NA_INTEGER
    G[cut + 3, :] = hib.NA_INTEGER
    before = grp.allreduces
    got = grp.predict_raw(G, want_dosage=True, want_prob=True)
    assert grp.allreduces - before == 2
    want = oracle.predict(oracle.flatten(model), G, vote_method=1, avx2=True, n_threads=8)
    R.assert_same(got, want, what=f"across the cut at {cut}")
    for s in grp.shards:
        assert s.handover_faults() == 0
    grp.close(); m.close()
