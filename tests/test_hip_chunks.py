"""The chunked tail of passes 1 and 2 at small shapes (DESIGN.md "The chunked tail, replayed and forced").

hibag_hip_test_set_chunking lowers the resident-workgroup figures a model launches with and sets its chunks per item, so that
cohorts of a few hundred samples run what otherwise takes thousands: every alignment of (items, resident workgroups), chunks
that are empty, items that are not cut, wavefronts that are not live, the storing / plain / FP4-only builds, pass 2's
classifier ranges with fewer classifiers than chunks and tiles without blocks.  Every case compares every output of every
sample with the oracle bit for bit (no tolerance anywhere), requires no failed hand-over, asserts through
hibag_hip_test_last_launch that the launch was cut the way the case is named, and runs the model with default chunking too.
No fault injection here and no repeated launches: tests/test_hip_status.py and the large shapes keep theirs."""

import numpy as np
import pytest

import launch_reference as LR
import layout_reference as R

pytestmark = pytest.mark.gpu

KEYS = ("h1", "h2", "prob", "matching", "dosage", "postprob")
NA = -2147483648
ENV = ("HIBAG_PASS2", "HIBAG_STORE_PAIRS", "HIBAG_PREBUILT_MB", "HIBAG_ENGINE")


@pytest.fixture(scope="module")
def hib():
    import hibag_amd
    assert "gfx950" in hibag_amd.hlaSetKernelTarget("hip")[0]
    return hibag_amd


def assert_same(got, want, what=""):
    for k in KEYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape, (what, k)
        if a.dtype.kind == "f":
            nan = np.isnan(a)
            same = np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
        else:
            same = np.array_equal(a, b)
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            i = tuple(bad[0]) if len(bad) else ()
            raise AssertionError(f"{what} {k}: {len(bad)} entries differ, first at {i}: hip={a[i]!r} oracle={b[i]!r}")


# ---- models and cohorts (built once; the oracle's answer once per model, cohort and vote method) -------------------------

def small_model(n_classifier=12, seed=5, **over):
    """The hla-a-small shape: one-step FP4 classifiers of 10 .. 24 SNPs, 14 alleles."""
    from hibag_amd import synth
    return synth.make_model("hla-a-small", seed=seed, n_classifier=n_classifier, wide_classifier=False, **over)


def cohort(model, founders, af, n, seed=9, bare=(2, 7)):
    """n samples: a ragged last group, sample 5 without any genotype, and the whole group 64 .. 127 without any SNP of the
    classifiers `bare` (nobody in that group uses them: their wavefront is not live in pass 1, and passed over in pass 2)."""
    from hibag_amd import synth
    assert n % 64 != 0 and n > 128
    G, _ = synth.make_samples(founders, af, n, seed=seed, miss=0.02)
    G[5, :] = NA
    for c in bare:
        if c < len(model.classifiers):
            G[64:128, np.asarray(model.classifiers[c].snpidx)] = NA
    return G


def kinds_model():
    """One classifier of every kind pass 1 walks in k_total: one-step FP4, int8 (31 and 32 SNPs), the vector engine (120 SNPs),
    no haplotypes at all, and three haplotypes (six pairs: a list of one block)."""
    from hibag_amd.model import Classifier
    counts = [14, 31, 120, 18, 16, 20, 32, 12]
    model, founders, af = small_model(len(counts), seed=17, n_snp=130, snp_counts=counts)
    c = model.classifiers[3]
    model.classifiers[3] = Classifier(snpidx=c.snpidx, freq=np.zeros(0), hla=np.zeros(0, np.int32), haplo=[])
    c = model.classifiers[4]
    model.classifiers[4] = Classifier(snpidx=c.snpidx, freq=np.asarray(c.freq[:3]) / np.sum(c.freq[:3]), hla=np.asarray(c.hla[:3]),
                                      haplo=list(c.haplo[:3]))
    return model, founders, af


def spare_alleles_model():
    """20 alleles of which the last six are carried by no classifier: tiles whose stream is empty in every classifier."""
    model, founders, af = small_model(6, seed=23)
    model.hla_allele = list(model.hla_allele) + [f"99:{i:02d}" for i in range(6)]
    return model, founders, af


UNDERFLOW_CLS, UNDERFLOW_SAMPLE = 5, 9


def underflow_model():
    """The mechanism of test_underflow_gives_nan_like_the_reference (a total so small that its reciprocal is infinite, so that
    0 * inf = NaN poisons the sample) inside a classifier k_total cuts: that test's 100-SNP classifier is walked by
    k_total_wide, never by a chunk, so here classifier 5 of the 12 -- one-step FP4 -- has its haplotype frequencies scaled
    by 1e-140: a sample six or more mismatches from its best pair has a total below 1e-308."""
    model, founders, af = small_model(12)
    c = model.classifiers[UNDERFLOW_CLS]
    c.freq = np.asarray(c.freq, np.float64) * 1e-140
    return model, founders, af


def underflow_cohort(model, founders, af, n):
    G = cohort(model, founders, af, n)
    idx = np.asarray(model.classifiers[UNDERFLOW_CLS].snpidx)
    H = np.array([[int(ch) for ch in h] for h in model.classifiers[UNDERFLOW_CLS].haplo])
    rng = np.random.default_rng(3)
    best, far = -1, None
    for _ in range(400):                       # a genotype vector far from every pair of its haplotypes
        g = rng.integers(0, 3, len(idx))
        two = H[:, None, :] + H[None, :, :]
        d = np.abs(two - g).sum(axis=2).min()
        if d > best:
            best, far = d, g
    assert best >= 8
    G[UNDERFLOW_SAMPLE, idx] = far
    return G


_models = {}


def case(name, n_samp=313):
    """(model, cohort) by name."""
    key = (name, n_samp)
    if key not in _models:
        make = {"small": small_model, "kinds": kinds_model, "two": lambda: small_model(2, seed=29), "spare": spare_alleles_model,
                "underflow": underflow_model, "other": lambda: small_model(9, seed=12, n_hla=11)}[name]
        model, founders, af = make()
        if name == "kinds":
            G = cohort(model, founders, af, n_samp, bare=(0, 7))       # (classifier 2 there holds nearly every SNP)
        else:
            G = (underflow_cohort if name == "underflow" else cohort)(model, founders, af, n_samp)
        if name == "kinds":
            # a classifier without haplotypes has total 0 for everybody who uses it (NaN, like the reference): the samples
            # from 128 on do not use it -- none of its SNPs -- and keep their numbers
            G[128:, np.asarray(model.classifiers[3].snpidx)] = NA
        _models[key] = (model, G)
    return _models[key]


_want = {}


def wanted(oracle, name, n_samp=313, vote=1):
    key = (name, n_samp, vote)
    if key not in _want:
        model, G = case(name, n_samp)
        _want[key] = oracle.predict(oracle.flatten(model), G, vote_method=vote, avx2=True, n_threads=8)
    return _want[key]


def set_env(monkeypatch, **env):
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


class Device:
    """A model on the device: first a call with default chunking (the same bits, and the launch's size: n, nx), then calls
    under the hook."""

    def __init__(self, hib, oracle, name, n_samp=313, vote=1):
        self.model, self.G = case(name, n_samp)
        self.want = wanted(oracle, name, n_samp, vote)
        self.vote, self.name = vote, name
        self.plan = R.export_plan(self.model)              # (under the environment of the moment, like the model below)
        self.dev = hib.hlaModelFromObj(self.model)
        self.base = self.run(0, 0, 0, "default chunking")
        assert self.base["p1_k"] == 1 and self.base["p2_k"] <= 1      # (a few hundred samples: nothing is cut by itself)

    def run(self, slots1, slots2, K, what):
        self.dev.set_chunking(slots1, slots2, K)
        got = self.dev.predict_raw(self.G, self.vote, want_dosage=True, want_prob=True)
        info = self.dev.last_launch()
        print(f"last_launch {self.name} n_samp={len(self.G)} {what}: " + " ".join(f"{k}={v}" for k, v in info.items()))
        assert_same(got, self.want, what)
        assert self.dev.status() == 0 and self.dev.handover_faults() == 0, what
        return info

    def close(self):
        self.dev.close()


def expect_total(info, n, slots, K, all_fp4, prebuilt):
    """Pass 1 was cut as the host arithmetic says for n items on `slots` resident workgroups -- and was cut at all."""
    P = LR.plan_total(n, slots, slots, K, all_fp4=all_fp4)
    assert {k: info["p1_" + k] for k in P} == P, (info, P)
    assert info["p1_kernel"] == 1 and info["p1_rest"] > 0 and info["p1_k"] == K and info["p1_n_whole"] + info["p1_rest"] == n
    assert info["p1_walk"] == (0 if not P["many"] else 2 if prebuilt else 1), info
    return P


def expect_accum(info, nx, sx, K):
    P = LR.plan_accum(nx, 8 * sx, K)
    assert {k: info["p2_" + k] for k in P} == P, (info, P)
    assert info["p2_kernel"] == 1 and info["p2_k"] == K and info["p2_n_whole"] < nx
    return P


def item_blocks(plan, n_item):
    """Blocks per work item of k_total (-1: a vector-engine item), from the exported plan's item list."""
    items = plan["item_whole" if n_item == plan["n_item_whole"] else "item_split"].reshape(-1, 4)[:n_item]
    cls = items[:, 0]
    return cls, np.where(plan["engine"][cls] > 0, plan["cls_nblk"][cls], -1)


# ---- pass 1: alignments of (items, resident workgroups) x chunks per item ---------------------------------------------------
# 12 one-step FP4 classifiers; 185 samples are one group quad (n = 12 items), 313 are two (n = 24).
# (samples, slots, n % slots, n_whole > 0, rest a multiple of 8)
ALIGN = [(185, 6, "0", True, False), (185, 4, "0", True, False), (185, 11, "1", False, False),
         (313, 5, "slots-1", True, False), (313, 8, "0", True, True), (313, 16, "other", False, True), (313, 23, "1", False, True)]


@pytest.mark.parametrize("K", [2, 3, 4, 12, 64])
@pytest.mark.parametrize("n_samp,slots,mod,whole,mult8", ALIGN)
def test_pass1_alignments(hib, oracle, monkeypatch, n_samp, slots, mod, whole, mult8, K):
    set_env(monkeypatch)
    D = Device(hib, oracle, "small", n_samp)
    try:
        n = D.base["p1_n"]
        assert n == 12 * ((n_samp + 255) // 256) and D.plan["all_fp4"] == 1 and D.plan["n_item_whole"] == 12
        assert {"0": n % slots == 0, "1": n % slots == 1, "slots-1": n % slots == slots - 1, "other": True}[mod]
        info = D.run(slots, 0, K, f"pass 1 slots={slots} K={K}")
        P = expect_total(info, n, slots, K, True, D.plan["p1_prebuilt"])
        assert (P["n_whole"] > 0) == whole and (P["rest"] % 8 == 0) == mult8 and info["p2_k"] == 1
        # what the launch ran, from the host replay: every cut item, a not-live wavefront among them, and for K = 64 empty chunks
        cls, nb = item_blocks(D.plan, 12)
        T = LR.pass1_table(P, n // 12, nb)
        assert np.count_nonzero(T["wait"] >= 0) == np.count_nonzero(T["post"] >= 0) > 0
        if K == 64:
            assert np.any(D.plan["cls_nblk"][cls] < K) and np.any(T["idle"] & T["cut"])
        if not whole:              # every item is cut: also those of classifiers 2 and 7, which group 64 .. 127 does not use
            assert {2, 7} <= set(cls[T["item"][T["cut"] & ~T["idle"]] // (n // 12)].tolist())
    finally:
        D.close()


def test_pass1_item_kinds_in_the_tail(hib, oracle, monkeypatch):
    """Every kind of work item in the chunked tail: one-step FP4, both int8 forms, a vector-engine item (not cut: its first chunk
    does all of it), a classifier without haplotypes (no blocks: the last chunk writes its total) and one of a single block."""
    set_env(monkeypatch)
    D = Device(hib, oracle, "kinds", 185)
    try:
        n = D.base["p1_n"]
        engines = [D.dev.engine(c)[0] for c in range(8)]
        assert engines[2] == "valu" and engines[1] == "i8" and engines[6] == "i8" and engines[0] == "fp4", engines
        assert D.plan["all_fp4"] == 0 and D.plan["n_valu"] == 1
        cls, nb = item_blocks(D.plan, n)
        assert np.any(nb < 0) and nb[cls == 3][0] == 0 and nb[cls == 4][0] == 1, (cls, nb)
        nan = np.isnan(D.want["postprob"]).all(axis=1)
        assert nan[[0, 1, 2, 30, 63]].all() and not nan[128:].any()        # (who uses the classifier without haplotypes is NaN, like the reference)
        for slots, K in ((n - 1, 3), (n - 1, 64), (max(n // 2, 1), 4)):
            info = D.run(slots, 0, K, f"kinds slots={slots} K={K}")
            P = expect_total(info, n, slots, K, False, D.plan["p1_prebuilt"])
            T = LR.pass1_table(P, 1, nb)
            tail = T["item"][(np.arange(T["grid"]) >= P["n_whole"]) & ~T["idle"]]
            if slots == n - 1:
                assert P["n_whole"] == 0 and set(cls[tail].tolist()) == set(cls.tolist())       # every kind is in the tail
                assert np.any(T["total"] & T["cut"] & (T["b1"] == 0) & (T["chunk"] == K - 1))     # the empty list's last chunk
    finally:
        D.close()


# ---- pass 1: the builds ---------------------------------------------------------------------------------------------------

def test_pass1_storing_build_resumes_inside_the_stored_cells(hib, oracle, monkeypatch):
    """HIBAG_PASS2=stream: pass 1 stores every cell sum, a chunk resumes at the row its first block's cells start at."""
    set_env(monkeypatch, HIBAG_PASS2="stream")
    D = Device(hib, oracle, "small")
    try:
        assert D.dev.stored_cells() > 0 and D.plan["store_cells"] == 1 and D.base["p1_store"] == 1 and D.base["p2_kernel"] == 2
        for slots, K, walk in ((16, 4, 0), (8, 3, 2)):                 # the general build and the FP4-only one, both storing
            info = D.run(slots, 8, K, f"stream slots={slots} K={K}")
            P = expect_total(info, 24, slots, K, True, D.plan["p1_prebuilt"])
            assert info["p1_store"] == 1 and info["p1_walk"] == walk and info["p2_kernel"] == 2
            cls, nb = item_blocks(D.plan, 12)
            T = LR.pass1_table(P, 2, nb)
            resumed = 0
            for b in np.nonzero(T["wait"] >= 0)[0]:
                c = cls[T["item"][b] // 2]
                row = D.plan["blk_close"][(int(D.plan["blk_off"][c]) - D.plan["p1_base"]) // 32 + T["b0"][b]]
                resumed += 0 < row < D.plan["cell_row"][c + 1] - D.plan["cell_row"][c]
            assert resumed > 0
    finally:
        D.close()


def test_pass1_plain_build(hib, oracle, monkeypatch):
    set_env(monkeypatch, HIBAG_PASS2="recompute")
    D = Device(hib, oracle, "small")
    try:
        assert D.dev.stored_cells() == 0 and D.plan["store_cells"] == 0
        info = D.run(16, 0, 4, "recompute slots=16 K=4")
        expect_total(info, 24, 16, 4, True, D.plan["p1_prebuilt"])
        assert info["p1_store"] == 0 and info["p1_walk"] == 0 and info["p2_kernel"] == 1
    finally:
        D.close()


@pytest.mark.parametrize("prebuilt", [True, False])
def test_pass1_fp4_only_builds(hib, oracle, monkeypatch, prebuilt):
    """n >= 2 * slots on a model whose items are all one-step FP4: the builds for six workgroups per CU, on prebuilt rows and
    (HIBAG_PREBUILT_MB=0) on rows generated from the haplotype table."""
    set_env(monkeypatch, **({} if prebuilt else {"HIBAG_PREBUILT_MB": "0"}))
    D = Device(hib, oracle, "small")
    try:
        assert D.plan["p1_prebuilt"] == int(prebuilt) and D.base["p1_many"] == 0
        for slots, K in ((12, 2), (5, 12)):
            info = D.run(slots, 0, K, f"fp4-only prebuilt={prebuilt} slots={slots} K={K}")
            expect_total(info, 24, slots, K, True, prebuilt)
            assert info["p1_many"] == 1 and info["p1_walk"] == (2 if prebuilt else 1)
    finally:
        D.close()


def test_the_vote_is_never_cut(hib, oracle, monkeypatch):
    set_env(monkeypatch)
    D = Device(hib, oracle, "small", vote=2)
    try:
        info = D.run(5, 8, 4, "vote slots=5 K=4")
        assert info["p1_vote"] == 1 and info["p1_k"] == 1 and info["p1_rest"] == 0 and info["p1_grid"] == info["p1_n"] == 24
        assert info["p2_launches"] == 0
    finally:
        D.close()


# ---- pass 2 -----------------------------------------------------------------------------------------------------------------

def pass2_slots(nx):
    """Resident workgroups per XCD for nx items: nx % sx == 0 with whole items in front, nx % sx != 0 without any, and with some."""
    exact = max(d for d in range(1, nx // 2 + 1) if nx % d == 0)
    some = next(s for s in (5, 4, 3, 7, 2, 6) if nx % s != 0 and nx > 2 * s)
    return [(exact, True, True), (nx - 1, False, False), (some, False, True)]


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("mode", ["hybrid", "recompute"])
def test_pass2_alignments(hib, oracle, monkeypatch, mode, K):
    """k_accum on a model of several tiles (14 alleles, 105 cells), 313 samples: five sample groups on eight XCDs, so three
    XCDs' workgroups have no samples and still hand over."""
    set_env(monkeypatch, HIBAG_PASS2=mode)
    D = Device(hib, oracle, "small")
    try:
        nx, n_tile, C = D.base["p2_nx"], D.plan["n_tile"], D.plan["n_classifier"]
        assert D.base["p2_kernel"] == 1 and nx == n_tile >= 7 and D.plan["store_cells"] == (2 if mode == "hybrid" else 0)
        cstart = D.plan["etile_cstart"].reshape(n_tile, C + 1)
        for sx, exact, whole in pass2_slots(nx):
            info = D.run(0, 8 * sx, K, f"pass 2 {mode} sx={sx} K={K}")
            P = expect_accum(info, nx, sx, K)
            assert (nx % sx == 0) == exact and (P["n_whole"] > 0) == whole and info["p1_k"] == 1
            T = LR.pass2_table(P, n_tile, cstart)
            assert np.count_nonzero(T["wait"] >= 0) == np.count_nonzero(T["post"] >= 0) > 0
    finally:
        D.close()


def test_pass2_fewer_classifiers_than_chunks(hib, oracle, monkeypatch):
    set_env(monkeypatch, HIBAG_PASS2="hybrid")
    D = Device(hib, oracle, "two")
    try:
        nx, n_tile = D.base["p2_nx"], D.plan["n_tile"]
        info = D.run(0, 8 * (nx - 1), 8, "two classifiers K=8")
        P = expect_accum(info, nx, nx - 1, 8)
        T = LR.pass2_table(P, n_tile, D.plan["etile_cstart"].reshape(n_tile, 3))
        assert np.any(T["idle"]) and np.any(T["wait"] >= 0)           # chunks without a classifier, and a hand-over all the same
    finally:
        D.close()


def test_pass2_empty_tiles_and_a_short_tile(hib, oracle, monkeypatch):
    """20 alleles, six of them in no classifier: tiles whose stream is empty (only the last chunk runs, on nothing), and a tile
    of fewer than 15 cells."""
    set_env(monkeypatch, HIBAG_PASS2="hybrid")
    D = Device(hib, oracle, "spare")
    try:
        nx, n_tile, C = D.base["p2_nx"], D.plan["n_tile"], D.plan["n_classifier"]
        cstart = D.plan["etile_cstart"].reshape(n_tile, C + 1)
        assert D.model.n_hla == 20 and np.any(cstart[:, C] == 0) and D.plan["tile_n"].min() < 15
        for sx, K in ((nx - 1, 3), (pass2_slots(nx)[0][0], 8)):
            info = D.run(0, 8 * sx, K, f"spare alleles sx={sx} K={K}")
            P = expect_accum(info, nx, sx, K)
            T = LR.pass2_table(P, n_tile, cstart)
            empty = cstart[T["item"] % n_tile, C] == 0
            assert np.any(T["cut"] & empty & ~T["idle"]) and np.all(T["chunk"][T["cut"] & empty & ~T["idle"]] == K - 1)
    finally:
        D.close()


# ---- both passes in one call ------------------------------------------------------------------------------------------------

BOTH = (5, 8 * 5, 3)          # resident workgroups of pass 1, of pass 2, chunks per item


def both_cut(dev):
    info = dev.last_launch()
    assert info["p1_k"] == 3 and info["p1_rest"] > 0 and info["p2_k"] == 3 and info["p2_n_whole"] < info["p2_nx"], info
    return info


def test_both_passes_back_to_back(hib, oracle, monkeypatch):
    """Two calls on one model: the second finds the flags of the first and tells them apart by their epoch."""
    set_env(monkeypatch)
    D = Device(hib, oracle, "small")
    try:
        first = D.run(*BOTH, "both passes, call 1")
        second = D.run(*BOTH, "both passes, call 2")
        for info in (first, second):
            expect_total(info, 24, 5, 3, True, D.plan["p1_prebuilt"])
            expect_accum(info, info["p2_nx"], 5, 3)
        assert second["p1_launches"] == first["p1_launches"] + 1 and second["p2_launches"] == first["p2_launches"] + 1
        # 0 restores every argument's default: the device's own figures again, nothing cut
        restored = D.run(0, 0, 0, "both passes, hook cleared")
        same = ("p1_slots", "p1_k", "p1_n_whole", "p1_grid", "p1_walk", "p2_sx", "p2_k", "p2_n_whole", "p2_grid")
        assert {k: restored[k] for k in same} == {k: D.base[k] for k in same}
        # a larger figure than the device reported is not taken: the hook only lowers
        raised = D.run(1 << 20, 1 << 20, 3, "both passes, slots above the device's")
        assert raised["p1_slots"] == D.base["p1_slots"] and raised["p2_sx"] == D.base["p2_sx"] and raised["p1_k"] == raised["p2_k"] == 1
    finally:
        D.close()


def test_both_passes_under_topk(hib, oracle, monkeypatch):
    from topk_reference import assert_topk_equal, topk
    set_env(monkeypatch)
    model, G = case("small")
    dev = hib.hlaModelFromObj(model)
    try:
        dev.set_chunking(*BOTH)
        got = dev.predict_topk(G, 4, 1)
        both_cut(dev)
        assert_topk_equal(got, topk(model, G, 4, vote=1), "top 4 under the hook")
        assert dev.status() == 0 and dev.handover_faults() == 0
    finally:
        dev.close()


def test_both_passes_under_given_with_full_sets(hib, oracle, monkeypatch):
    from given_reference import assert_given_equal, full_sets, given, pack
    set_env(monkeypatch)
    model, G = case("small")
    want = wanted(oracle, "small")
    allowed = full_sets(len(G), model.n_hla)
    dev = hib.hlaModelFromObj(model)
    try:
        dev.set_chunking(*BOTH)
        got = dev.predict_given(G, pack(allowed), 1, want_dosage=True)
        both_cut(dev)
        assert_given_equal(got, given(model, G, allowed, vote=1), "full sets under the hook")
        for key in ("h1", "h2", "prob", "dosage", "matching"):        # full sets: the plain call's outputs themselves
            assert np.array_equal(got[key], want[key], equal_nan=True), key
        assert dev.status() == 0 and dev.handover_faults() == 0
    finally:
        dev.close()


def test_both_passes_under_a_merge_of_two_models(hib, oracle, monkeypatch):
    """hlaPredictMerge of two models, both cut, against the composition the merge's own tests compare with:
    hlaPredMerge(hlaPredict(m1), hlaPredict(m2)) of the same models with default chunking.  (HIBAG_PASS2=hybrid: left to
    itself the second model, 11 alleles, stores every cell, and its pass 2 -- k_accum_cells -- has no chunks.)"""
    from hibag_amd import synth
    from test_hip_predmerge import assert_same as assert_merge_same, composed
    set_env(monkeypatch, HIBAG_PASS2="hybrid")
    objs = [case("small")[0], case("other")[0]]
    G = case("small")[1]
    for o in objs:
        o.hla_locus = "A"
    devs = [hib.hlaModelFromObj(o) for o in objs]
    try:
        snp = synth.as_snp_geno(objs[0], G)
        want, _ = composed(devs, snp, ret_postprob=True)
        for m in devs:
            info = m.last_launch()
            print("last_launch merge, composed with default chunking: " + " ".join(f"{k}={v}" for k, v in info.items()))
            assert info["p1_launches"] >= 1 and info["p1_k"] == 1 and info["p2_k"] <= 1      # (nothing cut in the yardstick)
            m.set_chunking(*BOTH)
        got = hib.hlaPredictMerge(devs, snp, ret_postprob=True, verbose=False)
        for m in devs:
            both_cut(m)
            assert m.status() == 0 and m.handover_faults() == 0
        assert_merge_same(got, want, True, True)
    finally:
        for m in devs:
            m.close()


# ---- an underflowing total in a last chunk -----------------------------------------------------------------------------------

def test_underflow_in_a_last_chunk(hib, oracle, monkeypatch):
    """Sample 9 is far from every haplotype pair of classifier 5, whose frequencies are tiny: its total there is so small
    that 1 / total is infinite, and the reference's 0 * inf = NaN poisons the sample's whole posterior.  Every item is cut
    (slots = n - 1), so the last chunk of classifier 5's item notes the infinite reciprocal."""
    set_env(monkeypatch)
    D = Device(hib, oracle, "underflow", 185)
    try:
        post = D.want["postprob"]
        assert np.isnan(post[UNDERFLOW_SAMPLE]).all() and D.want["h1"][UNDERFLOW_SAMPLE] == NA
        assert not np.isnan(post[[0, 1, 2, 70, 130, 184]]).any()
        for K in (3, 64):
            info = D.run(11, 0, K, f"underflow K={K}")
            P = expect_total(info, 12, 11, K, True, D.plan["p1_prebuilt"])
            assert P["n_whole"] == 0 and P["rest"] == 12
    finally:
        D.close()
