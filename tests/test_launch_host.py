"""The chunked tail of passes 1 and 2, replayed on the host (DESIGN.md "The chunked tail, replayed and forced"): the launch
arithmetic comes from the library's own functions (hibag_hip_test_plan_total / _accum: what the launchers call), the mapping of
a workgroup index to its work from tests/launch_reference.py, and the properties the hand-over scheme rests on are checked on
every launch of a sweep over items, resident workgroups, chunk counts, block counts and cost prefixes.  No GPU.

  1  partition     every item done exactly once; the non-empty chunks of a cut item tile its blocks / classifiers; each cut of
                   pass 2 is the first classifier boundary that reaches its share of the tile's blocks
  2  order, XCD    a waiting workgroup's poster has a smaller index, congruent mod 8
  3  completion    walked in index order every wait finds exactly its value in the flag; no flag value is posted twice
  4  bounds        every flag index below what a batch allocates; parked rows are the item's own
  5  no chunking   slots == 0, n <= slots, K == 1, and (pass 1) the majority vote: every item whole
"""

import numpy as np
import pytest

import launch_reference as LR


def _hibag():
    from hibag_amd import hibag
    return hibag


# ---- the arithmetic: the library's functions against the restatement, and what follows from the description ------------

def test_pass1_plan_over_the_whole_sweep():
    """Items 1 .. 200, slots 0 .. 64 (also no multiple of 8), every K once per (items, slots) residue class and K = 1, 2, 3, 64
    everywhere, both builds, vote and split."""
    H = _hibag()
    seen = dict(exact=0, plus_one=0, no_whole=0, ragged=0, many=0, off=0)
    for n in range(1, 201):
        for slots in range(0, 65):
            for K in {1, 2, 3, 64, 1 + (n * 7 + slots * 3) % 64}:
                for gx in (2,) if n % 16 == 0 else (1,):
                    got = H.plan_total(gx, n // gx, slots, 0, K)
                    want = LR.plan_total(n, slots, 0, K)
                    assert got == want, (n, slots, K, gx, got, want)
                    if slots == 0 or n <= slots or K == 1:                       # property 5
                        assert (got["k"], got["n_whole"], got["rest"], got["grid"]) == (1, n, 0, n)
                        seen["off"] += 1
                        continue
                    # the last, incomplete round and the full round before it; whole rounds in front
                    assert got["k"] == K and got["n_whole"] + got["rest"] == n
                    assert slots <= got["rest"] < 2 * slots and got["n_whole"] % slots == 0
                    assert got["stride"] % 8 == 0 and 0 <= got["stride"] - got["rest"] < 8
                    assert got["grid"] == got["n_whole"] + K * got["stride"]
                    seen["exact"] += n % slots == 0
                    seen["plus_one"] += n == slots + 1
                    seen["no_whole"] += got["n_whole"] == 0
                    seen["ragged"] += got["rest"] % 8 != 0
    # the switch of builds: the six-per-CU figures from two rounds of THEM on, for all-FP4 unsplit launches only
    for n in range(1, 201):
        for few, many in ((20, 24), (24, 20), (16, 0), (0, 16), (8, 64)):
            for fp4, split, vote in ((1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 1)):
                got = H.plan_total(1, n, few, many, 4, vote, fp4, split)
                assert got == LR.plan_total(n, few, many, 4, vote, fp4, split)
                is_many = bool(fp4 and not split and many > 0 and n >= 2 * many)
                assert got["many"] == is_many and got["slots"] == (many if is_many else few)
                if vote:
                    assert got["k"] == 1 and got["rest"] == 0 and got["grid"] == n      # property 5: the vote
                seen["many"] += is_many
    assert all(seen.values()), seen


def test_pass2_plan_over_the_whole_sweep():
    H = _hibag()
    seen = dict(exact=0, no_whole=0, whole=0)
    for nx in range(1, 65):
        for slots in list(range(0, 8 * 16 + 1, 8)) + [1, 7, 9, 15, 23, 100]:
            for K in {1, 2, 3, 8, 64, 1 + (nx * 5 + slots) % 64}:
                got = H.plan_accum(nx, slots, K)
                assert got == LR.plan_accum(nx, slots, K), (nx, slots, K)
                sx = slots // 8
                assert got["sx"] == sx
                if sx == 0 or nx <= sx or K == 1:                                # property 5
                    assert (got["k"], got["n_whole"], got["grid"]) == (1, nx, 8 * nx)
                    continue
                cut = nx - got["n_whole"]
                assert got["k"] == K and sx <= cut < 2 * sx and got["n_whole"] % sx == 0
                assert got["grid"] == 8 * (got["n_whole"] + K * cut)
                seen["exact"] += nx % sx == 0
                seen["no_whole"] += got["n_whole"] == 0
                seen["whole"] += got["n_whole"] > 0
    assert all(seen.values()), seen


def test_the_plan_entries_check_their_arguments():
    import ctypes as C
    from hibag_amd import _lib
    L = _lib.lib()
    info = _lib.LaunchInfo()
    ok = [2, 10, 16, 24, 4, 0, 1, 0]
    assert L.hibag_hip_test_plan_total(*ok, C.byref(info)) == 0 and info.p1_n == 20
    for at, bad in ((0, -1), (1, -1), (2, -1), (3, -1), (4, 0), (4, 65), (1, 1 << 30), (2, 1 << 25)):
        args = list(ok)
        args[at] = bad
        assert L.hibag_hip_test_plan_total(*args, C.byref(info)) == -1, (at, bad)
        assert "test_plan_total" in L.hibag_hip_last_error().decode()
    assert L.hibag_hip_test_plan_total(*ok, None) == -1
    assert L.hibag_hip_test_plan_accum(7, 16, 2, C.byref(info)) == 0 and info.p2_n_whole == 4 and info.p1_n == 0
    for bad in ((-1, 16, 2), (7, -1, 2), (7, 16, 0), (7, 16, 65), (1 << 22, 16, 2)):
        assert L.hibag_hip_test_plan_accum(*bad, C.byref(info)) == -1, bad
        assert "test_plan_accum" in L.hibag_hip_last_error().decode()
    assert L.hibag_hip_test_plan_accum(7, 16, 2, None) == -1


# ---- the properties ----------------------------------------------------------------------------------------------------

def _walk(T, n_flag):
    """Properties 2, 3 and the flag half of 4 on a table of either pass: the grid in index order with a flag array."""
    flags = np.full(n_flag, -1, np.int64)
    poster = np.full(n_flag, -1, np.int64)
    posted = set()
    for b in np.nonzero((T["wait"] >= 0) | (T["post"] >= 0))[0]:
        f = int(T["flag"][b])
        assert 0 <= f < n_flag, ("flag index", b, f, n_flag)
        if T["wait"][b] >= 0:
            assert flags[f] == T["wait"][b], ("a wait that does not find its value", int(b), int(flags[f]), int(T["wait"][b]))
            p = int(poster[f])
            assert p < b and (b - p) % 8 == 0, ("poster and waiter", p, int(b))
            assert T["row"][p] == T["row"][b], ("parked rows of another item", p, int(b))
        if T["post"][b] >= 0:
            key = (f, int(T["post"][b]))
            assert key not in posted, ("a flag value posted twice", int(b), key)
            posted.add(key)
            flags[f], poster[f] = T["post"][b], b


def check_pass1(P, gx, item_nb, n_samp=None):
    T = LR.pass1_table(P, gx, item_nb)
    n, n_whole, K = P["n"], P["n_whole"], P["k"]
    assert T["grid"] == P["grid"]
    busy = np.nonzero(~T["idle"])[0]
    assert np.all((T["item"][busy] >= 0) & (T["item"][busy] < n))
    assert np.array_equal(np.sort(T["item"][busy[T["total"][busy]]]), np.arange(n)), "every item's total written exactly once"
    # property 1: whole items are one workgroup ...
    assert np.array_equal(T["item"][:n_whole], np.arange(n_whole)) and not T["cut"][:n_whole].any() and not T["idle"][:n_whole].any()
    nb_of = np.asarray(item_nb)[np.arange(n) // gx]
    assert np.array_equal(T["b0"][:n_whole], np.zeros(n_whole, int)) and np.array_equal(T["b1"][:n_whole], np.maximum(nb_of[:n_whole], 0))
    assert np.all(T["wait"][:n_whole] < 0) and np.all(T["post"][:n_whole] < 0)
    # ... and the chunks of a cut item tile its blocks
    order = busy[busy >= n_whole]
    order = order[np.lexsort((T["chunk"][order], T["item"][order]))]
    by_item = np.split(order, np.nonzero(np.diff(T["item"][order]))[0] + 1) if len(order) else []
    assert len(by_item) == P["rest"]
    for blocks in by_item:
        li = int(T["item"][blocks[0]])
        nb = int(nb_of[li])
        if nb <= 0:                       # a vector-engine item, or an empty list: one workgroup, no hand-over
            assert len(blocks) == 1 and T["total"][blocks[0]] and T["wait"][blocks[0]] < 0 and T["post"][blocks[0]] < 0
            assert T["chunk"][blocks[0]] == (K - 1 if nb == 0 else 0)
            continue
        b0, b1 = T["b0"][blocks], T["b1"][blocks]
        assert b0[0] == 0 and b1[-1] == nb and np.all(b0 < b1) and np.array_equal(b1[:-1], b0[1:]), (li, nb, K, b0, b1)
        assert np.all(np.diff(blocks) > 0) and np.all(np.diff(blocks) % 8 == 0)          # property 2, also without a flag
        assert np.array_equal(T["wait"][blocks[1:]], b0[1:]) and T["wait"][blocks[0]] < 0
        assert np.array_equal(T["post"][blocks[:-1]], b1[:-1]) and T["post"][blocks[-1]] < 0
        assert len(blocks) == min(nb, K)
    n_flag1 = LR.n_flags(n_samp if n_samp is not None else gx * 256, 1, len(item_nb))[1]
    assert n_flag1 == gx * len(item_nb)
    _walk(T, n_flag1)
    return T


def check_pass2(P, n_tile, cstart, n_samp=None):
    cstart = np.asarray(cstart, np.int64).reshape(n_tile, -1)
    C = cstart.shape[1] - 1
    T = LR.pass2_table(P, n_tile, cstart)
    nx, n_whole, K = P["nx"], P["n_whole"], P["k"]
    assert T["grid"] == P["grid"] and nx % n_tile == 0
    busy = np.nonzero(~T["idle"])[0]
    # every (xcd, item) is finished exactly once
    assert np.array_equal(np.sort(T["row"][busy[T["final"][busy]]]), np.arange(8 * nx))
    head = busy[T["item"][busy] < n_whole]
    assert len(head) == 8 * n_whole and not T["cut"][head].any() and np.all(T["cb"][head] == 0) and np.all(T["ce"][head] == C)
    order = busy[T["item"][busy] >= n_whole]
    order = order[np.lexsort((T["chunk"][order], T["row"][order]))]
    by_item = np.split(order, np.nonzero(np.diff(T["row"][order]))[0] + 1) if len(order) else []
    assert len(by_item) == 8 * (nx - n_whole)
    for blocks in by_item:
        cum = cstart[int(T["item"][blocks[0]]) % n_tile]
        total = int(cum[C])
        cb, ce, k = T["cb"][blocks], T["ce"][blocks], T["chunk"][blocks]
        assert cb[0] == 0 and ce[-1] == C and np.all(cb < ce) and np.array_equal(ce[:-1], cb[1:]), (cum, K, cb, ce)
        assert np.all(np.diff(blocks) > 0) and np.all(np.diff(blocks) % 8 == 0) and np.all(T["xcd"][blocks] == T["xcd"][blocks[0]])
        # a cut is the FIRST boundary at which the chunks so far hold their share of the tile's blocks, (k + 1) / K of them
        for e, kk in zip(ce[:-1], k[:-1]):
            assert cum[e] * K >= total * (kk + 1) and (e == 0 or cum[e - 1] * K < total * (kk + 1)), (cum, K, int(kk), int(e))
        assert np.array_equal(T["wait"][blocks[1:]], cb[1:]) and T["wait"][blocks[0]] < 0
        assert np.array_equal(T["post"][blocks[:-1]], ce[:-1]) and T["post"][blocks[-1]] < 0
    n_flag2 = LR.n_flags(n_samp if n_samp is not None else 64 * 8 * 4 * (nx // n_tile), n_tile, 1)[0]
    assert n_flag2 == 8 * nx
    _walk(T, n_flag2)
    return T


def _pass1_cases():
    """(n, gx, slots, K): the named alignments, then a seeded sample of items 1 .. 200 x slots 0 .. 64 x K 1 .. 64."""
    cases = []
    for slots in (1, 7, 8, 9, 13, 16, 24, 63, 64):
        for n in sorted({slots, slots + 1, 2 * slots - 1, 2 * slots, 2 * slots + 1, 3 * slots, 3 * slots + 5}):
            if 1 <= n <= 200:
                cases += [(n, 1, slots, K) for K in (1, 2, 3, 12, 64)]
    rng = np.random.default_rng(20261)
    for _ in range(160):
        gx = int(rng.integers(1, 4))
        n = gx * int(rng.integers(1, 200 // gx + 1))
        cases.append((n, gx, int(rng.integers(0, 65)), int(rng.integers(1, 65))))
    cases += [(n, 1, 0, 4) for n in (1, 9, 200)]
    return cases


def test_pass1_properties_over_the_sweep():
    H = _hibag()
    rng = np.random.default_rng(20262)
    seen = dict(cut=0, empty_chunk=0, no_blocks=0, valu=0, pad=0, no_whole=0, exact=0, plus_one=0, whole=0)
    for n, gx, slots, K in _pass1_cases():
        P = H.plan_total(gx, n // gx, slots, 0, K)
        # block counts 0 .. 3 K (0, 1, K - 1, K, K + 1 often), and vector-engine items
        pick = np.array([0, 1, max(K - 1, 0), K, K + 1, 3 * K])
        item_nb = np.where(rng.random(n // gx) < 0.4, pick[rng.integers(0, 6, n // gx)], rng.integers(0, 3 * K + 1, n // gx))
        item_nb[rng.random(n // gx) < 0.1] = -1
        T = check_pass1(P, gx, item_nb)
        if P["rest"]:
            tail = np.arange(T["grid"]) >= P["n_whole"]
            seen["cut"] += 1
            seen["empty_chunk"] += bool(np.any(T["idle"] & T["cut"]))
            seen["no_blocks"] += bool(np.any(T["total"] & T["cut"] & (T["b1"] == 0)))
            seen["valu"] += bool(np.any(tail & ~T["cut"] & ~T["idle"]))
            seen["pad"] += bool(np.any(T["item"] < 0))
            seen["no_whole"] += P["n_whole"] == 0
            seen["exact"] += n % slots == 0
            seen["plus_one"] += n == slots + 1
        else:
            assert not T["cut"].any() and T["grid"] == n and not T["idle"].any()          # property 5
            seen["whole"] += 1
    assert all(v > 10 for v in seen.values()), seen


def _prefixes(rng, C, K):
    """Cost prefixes of C classifiers: random, with runs of equal values, all-zero, one heavy classifier, zeros at either end."""
    out = [np.zeros(C + 1, np.int64)]
    cost = rng.integers(0, 6, C)
    out.append(np.concatenate([[0], np.cumsum(cost)]))
    cost = rng.integers(0, 4, C) * (rng.random(C) < 0.4)               # runs of equal prefix values
    out.append(np.concatenate([[0], np.cumsum(cost)]))
    cost = np.zeros(C, np.int64)
    cost[rng.integers(0, C)] = int(rng.integers(1, 3 * K + 2))         # everything in one classifier
    out.append(np.concatenate([[0], np.cumsum(cost)]))
    cost = rng.integers(1, 9, C)
    cost[: C // 3] = 0                                                 # nothing in the first classifiers
    out.append(np.concatenate([[0], np.cumsum(cost)]))
    cost = rng.integers(1, 9, C)
    cost[C - C // 3:] = 0                                              # ... or in the last
    out.append(np.concatenate([[0], np.cumsum(cost)]))
    return out


def test_pass2_properties_over_the_sweep():
    H = _hibag()
    rng = np.random.default_rng(20263)
    seen = dict(cut=0, fewer_cls=0, empty_tile=0, whole=0, no_whole=0, exact=0, equal_run=0)
    cases = [(nx, sx, K) for nx in (1, 3, 7, 8, 9, 14, 21, 64) for sx in (0, 1, 2, 3, 7) for K in (1, 2, 3, 8, 64)]
    for _ in range(100):
        cases.append((int(rng.integers(1, 65)), int(rng.integers(0, 17)), int(rng.integers(1, 65))))
    for nx, sx, K in cases:
        P = H.plan_accum(nx, 8 * sx + int(rng.integers(0, 8)), K)
        n_tile = int(rng.choice([t for t in (1, 2, 3, 7, 8) if nx % t == 0]))
        C = int(rng.integers(1, 41))
        rows = _prefixes(rng, C, K)
        cstart = np.stack([rows[int(rng.integers(0, len(rows)))] for _ in range(n_tile)])
        T = check_pass2(P, n_tile, cstart)
        if P["n_whole"] < nx:
            seen["cut"] += 1
            seen["fewer_cls"] += C < K
            seen["empty_tile"] += bool(np.any(cstart[:, C] == 0))
            seen["no_whole"] += P["n_whole"] == 0
            seen["exact"] += nx % sx == 0
            seen["equal_run"] += bool(np.any(np.diff(cstart, axis=1) == 0))
        else:
            assert not T["cut"].any() and T["grid"] == 8 * nx and not T["idle"].any()     # property 5
            seen["whole"] += 1
    assert all(v > 10 for v in seen.values()), seen


@pytest.mark.parametrize("name", ["a_small", "hla_b"])
def test_real_layouts_tile_their_blocks_and_classifiers(name, monkeypatch):
    """cls_nblk and etile_cstart of two of the models tests/test_layout_host.py plans: pass 1's block ranges and pass 2's
    classifier ranges on them, every K, at slot figures that put every item into the tail."""
    import test_layout_host as TL
    H = _hibag()
    TL.set_env(monkeypatch, None, None, None, None)
    plan = TL.R.export_plan(TL.model_of(name)[0])
    assert plan["store_cells"] == 2                                     # (pass 2 is the block stream: etile_cstart is used)
    C, n_tile, n_item = plan["n_classifier"], plan["n_tile"], plan["n_item_whole"]
    cls = plan["item_whole"].reshape(-1, 4)[:n_item, 0]
    item_nb = np.where(plan["engine"][cls] > 0, plan["cls_nblk"][cls], -1)
    cstart = plan["etile_cstart"].reshape(n_tile, C + 1)
    assert np.all(np.diff(cstart.astype(np.int64), axis=1) >= 0) and np.all(cstart[:, 0] == 0)
    for K in (2, 3, 4, 8, 12, 64):
        for gx, slots in ((1, n_item - 1), (2, n_item), (3, 7)):
            P = H.plan_total(gx, n_item, slots, 0, K)
            assert P["rest"] > 0
            check_pass1(P, gx, item_nb, n_samp=gx * 256)
        for gq, sx in ((1, 5), (2, n_tile)):
            P = H.plan_accum(gq * n_tile, 8 * sx, K)
            assert P["n_whole"] < P["nx"]
            check_pass2(P, n_tile, cstart, n_samp=gq * 8 * 4 * 64)
