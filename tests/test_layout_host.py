"""The finalized predict layout, replayed on the host: the planning stages of hibag_model.hip run
without a device (hibag_hip_test_layout_plan), and tests/layout_reference.py reads their tables back the way the kernels do --
order, factors, headers, accounting, every index against the size of the array it addresses -- and recomputes the posterior
from them in float64 against the oracle, bit for bit.  No GPU."""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

import layout_reference as R

ENV = ("HIBAG_PASS2", "HIBAG_STORE_PAIRS", "HIBAG_PREBUILT_MB", "HIBAG_ENGINE")
PASS2 = (None, "stream", "hybrid", "recompute")
STORE_PAIRS = (None, "0", "3")
PREBUILT = (None, "0")
ENGINE = (None, "valu", "i8")
FULL = list(itertools.product(PASS2, STORE_PAIRS, PREBUILT, ENGINE))
# a diagonal through the settings for the larger models: every value of every setting at least once
DIAGONAL = [(PASS2[i % 4], STORE_PAIRS[i % 3], PREBUILT[i % 2], ENGINE[(i // 2) % 3]) for i in range(6)]
FUZZ_SEEDS = (90001, 90002, 90003, 90004, 90006, 90007, 90024, 90011)     # (90024: a "big" case of the campaign)
SEED_202699 = 202699


def _hib():
    import hibag_amd as hib
    return hib


def _widths():
    from hibag_amd import synth
    ks = list(range(1, 41)) + [63, 64, 65, 66, 96, 127, 128]
    return synth.make_model("hla-a-small", seed=77, n_classifier=len(ks), n_snp=160, snp_counts=ks, wide_classifier=False)[0]


def _only_wide():
    from hibag_amd import synth
    ks = [33, 40, 56, 57, 84, 85, 100, 112]
    return synth.make_model("hla-a-small", seed=31, n_classifier=len(ks), n_snp=130, snp_counts=ks, wide_classifier=False)[0]


def _campaign(seed):
    """(model, the campaign's HIBAG_STORE_PAIRS for it) of tests/test_hip_fuzz.py's wide campaign at `seed` (its cohort is not used)."""
    from test_hip_fuzz import _campaign_case
    rng = np.random.default_rng(seed)
    sp = str(int(rng.integers(0, 14))) if rng.random() < 0.5 else None
    model, _ = _campaign_case(_hib(), rng, big=(seed % 25 == 24))
    return model, sp


def _handmade(which):
    hib = _hib()
    rng = np.random.default_rng(5)

    def cls(k, n_snp, hla, freq=None):
        H = len(hla)
        f = rng.uniform(0.01, 1, H) if freq is None else np.asarray(freq, float)
        return hib.Classifier(snpidx=rng.choice(n_snp, k, replace=False).astype(np.int32), freq=f, hla=np.asarray(hla, np.int32),
                              haplo=["".join(rng.choice(["0", "1"], k)) for _ in range(H)])
    if which == "empty":         # classifiers without haplotypes (every engine), one haplotype, zero frequencies
        n_snp, nh = 130, 3
        c = [cls(5, n_snp, []), cls(4, n_snp, [1]), cls(40, n_snp, []), cls(6, n_snp, [0, 0, 2], [0.0, 0.3, 0.0]), cls(31, n_snp, [2]),
             cls(120, n_snp, []), cls(7, n_snp, [0, 1, 1, 1, 2, 2], [0.2, 0.0, 0.0, 0.0, 0.1, 0.3]), cls(60, n_snp, [1, 1, 2])]
    elif which == "one_allele":  # P = 1: one cell; 5 haplotypes = 15 pairs (odd), 1 haplotype = 1 pair
        n_snp, nh = 40, 1
        c = [cls(3, n_snp, [0]), cls(9, n_snp, [0] * 5), cls(32, n_snp, [0] * 2), cls(35, n_snp, [0] * 3), cls(12, n_snp, [0] * 9)]
    else:                        # two alleles, cells of 3, 2 and 1 pairs / 6, 9 and 6: odd pair counts
        n_snp, nh = 20, 2
        c = [cls(4, n_snp, [0, 0, 1]), cls(11, n_snp, [0, 0, 0, 1, 1, 1]), cls(1, n_snp, [0, 1]), cls(20, n_snp, [0] * 5 + [1] * 3)]
    return hib.HlaAttrBagObj(n_samp=0, n_snp=n_snp, hla_allele=[f"{i:02d}" for i in range(nh)], classifiers=c)


_cache = {}


def model_of(name):
    if name not in _cache:
        from hibag_amd import synth
        sp = None
        if name == "a_small":
            m = synth.make_model("hla-a-small")[0]
        elif name == "widths":
            m = _widths()
        elif name == "only_wide":
            m = _only_wide()
        elif name == "hla_b":
            m = synth.make_model("hla-b", n_classifier=8)[0]
        elif name == "alleles180":       # the model of test_many_alleles with fewer haplotypes: 16,290 cells, 1,086 tiles
            m = synth.make_model("hla-b", seed=21, n_hla=180, n_haplo=150, n_classifier=4, n_snp=120)[0]
        elif name == "drb1":
            m = synth.make_model("hla-drb1", n_classifier=3)[0]
        elif name.startswith("fuzz"):
            m, sp = _campaign(int(name[4:]))
        else:
            m = _handmade(name)
        _cache[name] = (m, R.Model(m), sp)
    return _cache[name]


def set_env(monkeypatch, pass2, store_pairs, prebuilt, engine):
    for key, v in zip(ENV, (pass2, store_pairs, prebuilt, engine)):
        monkeypatch.setenv(key, v) if v is not None else monkeypatch.delenv(key, raising=False)
    return R.Settings.from_env(os.environ)


def audited(monkeypatch, name, setting):
    obj, model, _ = model_of(name)
    S = set_env(monkeypatch, *setting)
    plan = R.export_plan(obj)
    return plan, R.audit(plan, model, S), S


def cohort(obj, seed, n=70):
    """~70 samples: random calls with 2-5 % missing, an all-NA row, out-of-range codes (-1, 3), and samples that are the sum
    of two haplotypes of one classifier (so that somebody matches)."""
    rng = np.random.default_rng(seed)
    S = obj.n_snp
    G = rng.integers(0, 3, (n, S)).astype(np.int32)
    with_h = [c for c in obj.classifiers if len(c.freq)]
    for i in range(20, min(n, 50)):
        c = with_h[i % len(with_h)] if with_h else None
        if c is not None:
            H0 = np.array([[int(ch) for ch in h] for h in c.haplo], np.int32).reshape(len(c.freq), -1)
            a, b = rng.integers(0, len(H0), 2)
            G[i, np.asarray(c.snpidx)] = H0[a] + H0[b]
    G[rng.random(G.shape) < rng.uniform(0.02, 0.05)] = R.NA_INTEGER
    G[5:9][rng.random((4, S)) < 0.1] = -1
    G[9:13][rng.random((4, S)) < 0.1] = 3
    G[3, :] = R.NA_INTEGER
    G[4, : S // 2] = R.NA_INTEGER
    return G


def same_posterior(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


# ---- rules A - G -----------------------------------------------------------------------------------------------------

SMALL = ("a_small", "empty", "one_allele", "two_alleles")
LARGE = ("widths", "only_wide", "hla_b", "alleles180", "drb1") + tuple(f"fuzz{s}" for s in FUZZ_SEEDS + (SEED_202699,))


@pytest.mark.parametrize("name", SMALL)
def test_small_models_under_every_setting(name, monkeypatch):
    modes = set()
    for setting in FULL:
        plan, a, _ = audited(monkeypatch, name, setting)
        assert not a.findings, (name, setting, a.findings[:5])
        modes.add(plan["store_cells"])
    print(name, "store modes", modes)
    assert {1, 2} <= modes


@pytest.mark.parametrize("name", LARGE)
def test_large_models_on_a_diagonal_of_settings(name, monkeypatch):
    _, _, sp = model_of(name)
    settings = list(DIAGONAL)
    if name.startswith("fuzz"):
        settings = [(None, sp, None, None)] + settings[:3]            # (the campaign's own store threshold first)
    for setting in settings:
        plan, a, _ = audited(monkeypatch, name, setting)
        assert not a.findings, (name, setting, a.findings[:5])
    if name == "drb1":
        assert audited(monkeypatch, name, (None, None, None, None))[0]["store_cells"] == 1        # the DRB1 shape: every cell stored
    if name == "alleles180":
        assert plan["n_tile"] > 1000
    if name == "only_wide":
        plan = audited(monkeypatch, name, (None, None, None, None))[0]
        assert plan["n_wide"] == 8 and plan["n_wide_scan"] == 0 and plan["second_pass_pairs"] == 0
    if name == "widths":
        plan = audited(monkeypatch, name, (None, None, None, None))[0]
        assert plan["n_wide"] == 13 and plan["n_wide_scan"] == 0 and plan["n_wide_seg"] == 13 and plan["n_valu"] == 2
        assert set(plan["engine"].tolist()) == {0, 1, 2, 3}


def test_the_models_reach_every_branch(monkeypatch):
    """What the model list is there for: a split vector-engine classifier, prebuilt rows on and off, blocks that carry stored sums only,
    every store mode, classifiers whose operand row is 0 because they have none."""
    seen = dict(split=False, p1_prebuilt=set(), sums_only=False, valu_last=False, segments=False)
    for name in ("widths", "a_small", "hla_b", f"fuzz{SEED_202699}"):
        for setting in [(None, None, None, None), (None, "0", "0", None)]:
            if name.startswith("fuzz"):
                setting = (None, model_of(name)[2], None, None)
            plan, a, _ = audited(monkeypatch, name, setting)
            assert not a.findings
            seen["split"] |= plan["n_split"] > 0
            seen["segments"] |= plan["n_wide_scan"] > 0 and plan["n_wide_seg"] > plan["n_wide"]       # a classifier of several K steps in several segments
            seen["p1_prebuilt"].add(plan["p1_prebuilt"])
            eb = plan["estream_blocks"]
            hd = plan["ehdr"].reshape(eb, 8)
            seen["sums_only"] |= bool(np.any((hd[:, 6] >> 28 == 0) & ((hd[:, 1] >> 25) & 15 > 0)))
            seen["valu_last"] |= plan["engine"][plan["n_classifier"] - 1] == 0 and plan["store_cells"] == 2
    assert seen == dict(split=True, p1_prebuilt={0, 1}, sums_only=True, valu_last=True, segments=True), seen


# ---- rule H ----------------------------------------------------------------------------------------------------------

H_CASES = [(n, s) for n in ("a_small", "empty", "one_allele", "two_alleles") for s in
           [(p, sp, None, e) for p in PASS2 for sp, e in ((None, None), ("0", "i8"), ("3", "valu"))]] + \
          [("widths", (None, None, None, None)), ("widths", ("hybrid", "3", "0", None)), ("only_wide", (None, None, None, None)),
           ("only_wide", ("stream", None, None, None)), ("hla_b", (None, None, None, None)), ("hla_b", ("recompute", None, None, None)),
           ("fuzz90001", (None, "0", None, None)), ("fuzz90002", ("hybrid", "3", None, None)), ("fuzz90003", (None, None, None, "i8"))]


def test_the_posterior_replayed_from_the_lists_is_the_oracles(oracle, monkeypatch):
    want = {}
    for name, setting in H_CASES:
        obj, _, _ = model_of(name)
        plan, a, _ = audited(monkeypatch, name, setting)
        assert not a.findings, (name, setting, a.findings[:5])
        if name not in want:
            G = cohort(obj, 11)
            want[name] = (G, oracle.predict(oracle.flatten(obj), G, vote_method=1, want_dosage=False)["postprob"])
        G, post = want[name]
        p1, p2 = R.replay(a, G)
        assert same_posterior(p1, post), (name, setting, "pass 1's lists")
        assert same_posterior(p2, post), (name, setting, "pass 2's view")
    assert np.isnan(want["a_small"][1]).any() or True          # (all-NA rows: NaN or zero rows, whatever the oracle says)


# ---- the export itself -----------------------------------------------------------------------------------------------

def test_planning_leaves_the_model_unfinalized_and_usable(monkeypatch):
    from hibag_amd import _lib
    set_env(monkeypatch, None, None, None, None)
    L = _lib.lib()
    obj = model_of("a_small")[0]
    h = R.new_model_handle(obj)
    try:
        p1, p2 = R.plan_of_handle(h), R.plan_of_handle(h)
        assert p1.keys() == p2.keys() and all(np.array_equal(p1[k], p2[k]) for k in p1)
        # the room of every array covers it, with the minima upload_layout reserves
        assert p1["room:parow"] >= max(p1["parow"].nbytes, 1024) and p1["room:wide_seg"] >= 4 and p1["bt_rows_alloc"] == p1["bt_rows"] + 2
        # still a model under construction: another classifier goes in, and the plan follows
        c = obj.classifiers[0]
        strs = (C.c_char_p * len(c.haplo))(*[s.encode() for s in c.haplo])
        idx, fr, hla = np.ascontiguousarray(c.snpidx, np.int32), np.ascontiguousarray(c.freq), np.ascontiguousarray(c.hla, np.int32)
        assert L.hibag_hip_model_add_classifier(h, len(idx), idx.ctypes.data_as(C.c_void_p), len(fr), fr.ctypes.data_as(C.c_void_p),
                                                hla.ctypes.data_as(C.c_void_p), strs) == 0
        assert R.plan_of_handle(h)["n_classifier"] == p1["n_classifier"] + 1
    finally:
        L.hibag_hip_model_free(h)
    assert not L.hibag_hip_test_layout_plan(None) and b"NULL" in L.hibag_hip_last_error()
    assert L.hibag_hip_test_layout_count(None) == 0
    assert L.hibag_hip_test_layout_get(None, 0, None, None, None, None) == -1


def test_a_plan_the_stages_reject_returns_their_error(monkeypatch):
    """32,769 one-step classifiers: the last one's operand row does not fit the 16 bits the block headers have for it."""
    from hibag_amd import _lib
    set_env(monkeypatch, None, None, None, None)
    L = _lib.lib()
    h = C.c_void_p(L.hibag_hip_model_new(1, 1))
    try:
        idx, fr, hla = np.zeros(1, np.int32), np.ones(1), np.zeros(1, np.int32)
        strs = (C.c_char_p * 1)(b"1")
        for _ in range(32769):
            assert L.hibag_hip_model_add_classifier(h, 1, idx.ctypes.data_as(C.c_void_p), 1, fr.ctypes.data_as(C.c_void_p), hla.ctypes.data_as(C.c_void_p), strs) == 0
        assert not L.hibag_hip_test_layout_plan(h)
        assert b"too many classifiers for the matrix engine's operand rows" in L.hibag_hip_last_error()
    finally:
        L.hibag_hip_model_free(h)


# ---- the audit has teeth -----------------------------------------------------------------------------------------------

def _p1_cell(a, min_slots, stored=None, skip=0):
    """(classifier, first slot, last slot) -- dword offsets in plist -- of a pass-1 cell of a one-step classifier with at least
    `min_slots` slots (and the given STORE state)."""
    for c, p in a.p1.items():
        if a.steps[c] != 1:
            continue
        n = np.diff(p["estart"])
        for i in np.nonzero(n >= min_slots)[0]:
            if stored is not None and bool(p["flagged"][i]) != stored:
                continue
            if skip:
                skip -= 1
                continue
            return c, p["off"] + int(p["real"][p["estart"][i]]), p["off"] + int(p["real"][p["estart"][i + 1] - 1])
    raise AssertionError("no such cell")


def _corruptions(plan, a):
    """name -> (rule the audit must report, function that corrupts a copy of the plan in one place)."""
    eb = plan["estream_blocks"]
    hd = plan["ehdr"].reshape(eb, 8)
    cnt = (hd[:, 1] >> 25) & 15
    b_sum = int(np.nonzero((cnt > 0) & (cnt < 7))[0][0])                 # a block with stored sums
    b_mid = int(np.nonzero(hd[:, 6] >> 28)[0][3])                         # a block with slots
    c, s0, s1 = _p1_cell(a, 4, stored=False)
    _, t0, t1 = _p1_cell(a, 2, stored=True)
    _, u0, u1 = _p1_cell(a, 2, stored=False, skip=1)
    close = int(np.nonzero(plan["blk_close"])[0][0])

    def swap(q): q["plist"][[s0 + 1, s0 + 2]] = q["plist"][[s0 + 2, s0 + 1]]
    def end_cleared(q): q["plist"][s1] &= 0x7FFFFFFF
    def end_even(q): q["plist"][s1] &= 0x7FFFFFFF; q["plist"][s1 - 1] |= 0x80000000
    def store_moved(q): q["plist"][t1] &= ~np.uint32(R.STORE); q["plist"][u1] |= R.STORE
    def pfac_ulp(q): q["pfac"][s0] = np.nextafter(q["pfac"][s0], 2.0)
    def stored_row(q): q["ehdr"][8 * b_sum + 1] += 1
    def operand_row(q): q["ehdr"][8 * b_mid + 7] = (q["ehdr"][8 * b_mid + 7] & 0xFFFF) | (q["bt_rows_alloc"] << 16)
    def stored_count(q): q["ehdr"][8 * b_sum + 1] += 1 << 25
    def bit29(q): q["ehdr"][8 * b_mid + 1] ^= 1 << 29
    def cstart(q): q["etile_cstart"][3] += 1
    def blk_close(q): q["blk_close"][close] += 1
    def nibble(q): q["hap"][q["hap_off"][c] + 12] ^= 0x20
    def parow(q): i = int(np.nonzero(q["parow"])[0][100]); q["parow"][i] ^= 0x100
    def slack(q): q["plist"] = q["plist"][:-32]; q["pfac"] = q["pfac"][:-32]; q["phdr"] = q["phdr"][:-4]
    def cls_cnt(q): q["cls_cnt"][1] += 1
    return {"two slots swapped inside a cell": ("B.order", swap), "an END flag cleared": ("B.order", end_cleared),
            "an END moved to an even slot": ("B.pad", end_even), "a STORE flag moved to another cell": ("B.store", store_moved),
            "one pfac changed by one ulp": ("B.pfac", pfac_ulp), "a header's stored row + 1": ("C.ehdr", stored_row),
            "a header's operand row set to the rows of the batch's array": ("G.bounds", operand_row), "a stored count + 1": ("C.ehdr", stored_count),
            "bit 29 flipped": ("C.ehdr", bit29), "an etile_cstart entry shifted by one": ("C.cstart", cstart),
            "a blk_close entry + 1": ("B.blk_close", blk_close), "a table nibble changed": ("A.hap", nibble),
            "a parow dword changed": ("F.parow", parow), "the last slack block removed": ("G.bounds", slack),
            "a cls_cnt entry changed": ("E.cls_cnt", cls_cnt)}


def test_every_corruption_is_reported_under_its_rule(monkeypatch):
    _, model, _ = model_of("a_small")
    plan, a, S = audited(monkeypatch, "a_small", (None, None, None, None))
    assert not a.findings and plan["store_cells"] == 2 and plan["p1_prebuilt"] == 1
    todo = _corruptions(plan, a)
    assert len(todo) == 15
    for what, (rule, corrupt) in todo.items():
        q = plan.copy()
        corrupt(q)
        got = R.audit(q, model, S).rules()
        assert rule in got, (what, rule, got)


def test_further_corruptions_reach_the_other_rules(monkeypatch):
    """One corruption for each rule the list above does not touch."""
    _, model, _ = model_of("a_small")
    plan, a, S = audited(monkeypatch, "a_small", (None, None, None, None))
    eb = plan["estream_blocks"]
    b_mid = int(np.nonzero(plan["ehdr"].reshape(eb, 8)[:, 6] >> 28)[0][3])
    closing = int(np.nonzero(plan["ehdr"].reshape(eb, 8)[:, 0])[0][5])              # a block in which a cell closes

    def estream_swap(q): q["plist"][[32 * b_mid, 32 * b_mid + 1]] = q["plist"][[32 * b_mid + 1, 32 * b_mid]]
    def ctile_row(q): q["ctile"][8 * 7 + 5] += 1
    def cell_row(q): q["cell_row"][3:] += 1
    def closing_row(q):
        w0 = int(q["ehdr"][8 * closing]); i = (w0 & -w0).bit_length() - 1           # the first closing slot's field
        q["ehdr"][8 * closing + 4 + i // 16] ^= 1 << (4 * ((i // 2) % 8))
    def n_valid(q): q["phdr"][4 * (plan["p1_base"] // 32) + 2] -= 1
    def tile_meta(q): q["tile_meta"][1] += 1
    def bt_row(q): q["bt_row"][2] += 2
    for what, (rule, corrupt) in {"two E-stream slots swapped": ("C.slots", estream_swap), "a ctile stored row + 1": ("C.ctile", ctile_row),
                                  "cell_row shifted": ("D.cells", cell_row), "a closing cell's tile row changed": ("D.cells", closing_row),
                                  "a phdr n_valid - 1": ("B.phdr", n_valid), "a tile_meta word changed": ("E.tile_meta", tile_meta),
                                  "a bt_row + 2": ("A.engine", bt_row)}.items():
        q = plan.copy()
        corrupt(q)
        got = R.audit(q, model, S).rules()
        assert rule in got, (what, rule, got)
    _, model, _ = model_of("widths")
    plan, a, S = audited(monkeypatch, "widths", (None, None, None, None))
    valu = int(np.nonzero(plan["engine"][:model.C] == 0)[0][0])

    def record(q): q["stream"][q["stream_off"][valu] + 5] ^= 1
    def item(q): q["item_split"][2] -= 1
    def segment(q): q["wide_seg"][1] += 1
    for what, (rule, corrupt) in {"a record's bit flipped": ("E.stream", record), "a work item one cell short": ("E.items", item),
                                  "a segment's first stored row + 1": ("B.wide", segment)}.items():
        q = plan.copy()
        corrupt(q)
        got = R.audit(q, model, S).rules()
        assert rule in got, (what, rule, got)


def test_the_operand_row_past_the_batchs_array_is_caught_on_seed_202699(monkeypatch):
    """The fault of tests/test_hip_fuzz.py::test_campaign_case_with_vector_engine_classifiers_last, on the host: the model's last
    classifiers run on the vector engine and have no operand rows; the headers of their stored-sums-only blocks must name row 0, and the
    batch's array has two rows to spare.  Naming the row behind the model's last -- what the headers did -- is a wrong header word now
    (rule C) and inside the array thanks to the spare rows; naming the row behind the array is out of bounds (rule G)."""
    name = f"fuzz{SEED_202699}"
    obj, model, sp = model_of(name)
    assert sp == "0" and len(obj.classifiers) == 59 and len(obj.classifiers[-1].snpidx) == 120
    plan, a, S = audited(monkeypatch, name, (None, sp, None, None))
    assert not a.findings
    assert plan["store_cells"] == 2 and plan["engine"][58] == 0 and plan["bt_row"][58] == plan["bt_rows"]
    eb = plan["estream_blocks"]
    hd = plan["ehdr"].reshape(eb, 8)
    last = np.nonzero((hd[:, 7] & 0xFFFF) == 58)[0]
    assert len(last) and np.all(hd[last, 7] >> 16 == 0) and np.all(hd[last, 6] >> 28 == 0) and np.all((hd[last, 1] >> 25) & 15 > 0)
    b = int(last[0])
    for row, rule in ((plan["bt_rows"], "C.ehdr"), (plan["bt_rows"] + 1, "G.bounds"), (plan["bt_rows_alloc"], "G.bounds")):
        q = plan.copy()
        q["ehdr"][8 * b + 7] = 58 | (row << 16)
        q["ehdr"][8 * (b - 1) + 2] = q["ehdr"][8 * b + 7]             # (the copy in the header before it, as the layout would carry it)
        got = R.audit(q, model, S)
        assert rule in got.rules(), (row, rule, got.findings[:5])
        if rule == "G.bounds":
            assert any(r == "G.bounds" and "operand row" in m for r, m in got.findings)
