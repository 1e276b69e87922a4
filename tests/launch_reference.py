"""How a workgroup index becomes work in the chunked passes 1 and 2, restated for the tests (DESIGN.md "The chunked tail,
replayed and forced").

Written from the descriptions in ``hibag_amd/csrc/hibag_k_pass1.h`` ("hand-overs", and the comment in front of ``k_total``)
and ``hibag_k_pass2.h`` (the grid comment in front of ``k_accum`` and the classifier range at its top), in plain numpy, one
array entry per workgroup of a launch.  ``tests/test_launch_host.py`` checks the scheme's invariants on these tables;
``tests/test_hip_chunks.py`` uses them to say which path a device case takes.

Pass 1.  Workgroups ``[0, n_whole)`` take item ``b`` whole.  Behind them the other ``rest`` items go in ``K`` chunks along
their block lists: all first chunks, then all second chunks, ..., each round ``stride`` workgroups long (``rest`` rounded up
to a multiple of 8, so the chunks of an item share an XCD; the workgroups past ``rest`` in a round are idle).  Chunk ``k`` of
an item of ``nb`` blocks takes blocks ``[nb k / K, nb (k + 1) / K)``; an empty range does nothing at all -- except the last
chunk of an item without blocks, which still writes the item's total.  Only matrix-engine items are cut: a vector-engine
item is done whole by its first chunk.  A chunk that does not start at block 0 waits until the item's flag shows its first
block; a chunk that is not the last posts the block it stopped at, after parking its sums in the item's own rows.

Pass 2.  Workgroup ``8 w + x`` is number ``w`` of XCD ``x``; per XCD, numbers ``[0, n_whole)`` take item ``w`` whole, behind
them the other ``nx - n_whole`` items go in ``K`` chunks, round after round.  An item is (group quad, tile), tile fastest;
chunk ``k`` takes the classifiers from the first one whose cost prefix in the tile reaches ``ceil(total k / K)`` up to the
first one that reaches ``ceil(total (k + 1) / K)``; chunk 0 starts at classifier 0, the last chunk ends at ``C``.  An empty
range does nothing.  A chunk that does not start at classifier 0 waits for its first classifier on the item's flag; one that
does not end at ``C`` parks the tile's sums and posts where it stopped.
"""

from __future__ import annotations

import numpy as np

WAVES1 = 4          # wavefronts (sample groups of 64) per workgroup of pass 1
WAVES2 = 4          # ... and of pass 2
XCDS = 8


# ---- the launch arithmetic ---------------------------------------------------------------------------------------------

def plan_total(n: int, slots_few: int, slots_many: int, k_req: int, vote=False, all_fp4=False, split=False) -> dict:
    """More items than resident workgroups: the last, incomplete round and the full round before it go in K chunks."""
    many = bool(all_fp4 and not split and slots_many > 0 and n >= 2 * slots_many)
    slots = slots_many if many else slots_few
    out = dict(n=n, slots=max(slots, 0), k=1, n_whole=n, rest=0, stride=8, many=int(many))
    if not vote and k_req > 1 and slots > 0 and n > slots:
        rest = n % slots + slots
        out.update(k=k_req, rest=rest, n_whole=n - rest, stride=-(-rest // 8) * 8)
    out["grid"] = out["n_whole"] + (out["k"] * out["stride"] if out["rest"] else 0)
    return out


def plan_accum(nx: int, slots: int, k_req: int) -> dict:
    sx = max(slots, 0) // XCDS
    out = dict(nx=nx, sx=sx, k=1, n_whole=nx)
    if k_req > 1 and sx > 0 and nx > sx:
        out.update(k=k_req, n_whole=nx - (nx % sx + sx))
    out["grid"] = XCDS * (out["n_whole"] + out["k"] * (nx - out["n_whole"]))
    return out


def n_flags(n_samp: int, n_tile: int, n_item: int) -> tuple:
    """(flags of pass 2, flags of pass 1) a batch of ``n_samp`` samples allocates: one per pass-2 item (8 XCDs x group quads
    x tiles), then one per pass-1 item (group quads x the model's items)."""
    groups = -(-max(n_samp, 1) // 64)
    n_gq2 = -(-(-(-groups // XCDS)) // WAVES2)
    return XCDS * n_gq2 * max(n_tile, 1), -(-groups // WAVES1) * max(n_item, 1)


# ---- pass 1 ------------------------------------------------------------------------------------------------------------

def pass1_table(plan: dict, gx: int, item_nb) -> dict:
    """One entry per workgroup of a pass-1 launch.  ``plan``: n, n_whole, rest, stride, k (and grid); ``gx``: group quads;
    ``item_nb[i]``: blocks of the model's item i (its classifier's list), -1 for a vector-engine item.

    item      the work item (model item x group quad; -1: a workgroup past `rest` in its round)
    chunk     k (0 for undivided items)
    b0, b1    the block range
    idle      returns before doing, waiting for or posting anything
    first, last
    flag      index among the pass-1 flags (-1: none)
    wait      the progress it waits for (-1: none);  post: the progress it posts (-1: none)
    total     writes the item's total
    row       the (model item, group quad) whose rows it parks into or reads parked sums from: li itself
    """
    item_nb = np.asarray(item_nb, np.int64)
    n, n_whole, rest, stride, K = (int(plan[k]) for k in ("n", "n_whole", "rest", "stride", "k"))
    grid = n_whole + (K * stride if rest else 0)
    b = np.arange(grid, dtype=np.int64)
    tail = b >= n_whole
    jj = np.where(tail, b - n_whole, 0)
    k = jj // max(stride, 1)
    j = jj - k * stride
    pad = tail & (j >= rest)
    li = np.where(tail, n_whole + j, b)
    li = np.where(pad, -1, li)
    nb = np.where(pad, 0, item_nb[np.where(pad, 0, li) // gx])
    matrix = nb >= 0
    cut = tail & ~pad & matrix
    b0 = np.where(cut, nb * k // K, 0)
    b1 = np.where(cut, nb * (k + 1) // K, np.maximum(nb, 0))
    empty = cut & (b0 >= b1) & ~((k == K - 1) & (nb == 0))
    later_valu = tail & ~pad & ~matrix & (k > 0)
    idle = pad | empty | later_valu
    first = b0 == 0
    last = ~cut | (k == K - 1)
    return dict(grid=grid, item=li, chunk=np.where(tail, k, 0), b0=b0, b1=b1, idle=idle, first=first, last=last, cut=cut,
                flag=np.where(tail & ~pad, li - n_whole, -1), wait=np.where(~idle & ~first, b0, -1),
                post=np.where(~idle & ~last, b1, -1), total=~idle & last, row=li)


# ---- pass 2 ------------------------------------------------------------------------------------------------------------

def chunk_bound(cum, target: int) -> int:
    """First classifier of a tile whose cost prefix reaches ``target`` (``cum``: C + 1 entries; C if none of 0 .. C - 1 does)."""
    return int(np.searchsorted(np.asarray(cum)[:-1], target, side="left"))


def chunk_range(cum, k: int, K: int) -> tuple:
    """Classifiers [cb, ce) of chunk k of K of an item whose tile has the cost prefix ``cum``."""
    C = len(cum) - 1
    total = int(cum[C])
    cb = chunk_bound(cum, (total * k + K - 1) // K) if k > 0 else 0
    ce = chunk_bound(cum, (total * (k + 1) + K - 1) // K) if k < K - 1 else C
    return cb, ce


def pass2_table(plan: dict, n_tile: int, cstart) -> dict:
    """One entry per workgroup of a pass-2 launch.  ``plan``: nx, n_whole, k; ``cstart``: [n_tile][C + 1] cost prefixes.

    xcd, item, chunk, cb, ce, idle, flag (-1: none), wait, post (-1: none), final (writes the item's sums for good),
    row (xcd, item): whose parked sums it reads or writes.
    """
    cstart = np.asarray(cstart, np.int64).reshape(n_tile, -1)
    C = cstart.shape[1] - 1
    nx, n_whole, K = int(plan["nx"]), int(plan["n_whole"]), int(plan["k"])
    r = nx - n_whole
    grid = XCDS * (n_whole + K * r)
    b = np.arange(grid, dtype=np.int64)
    xcd, w = b % XCDS, b // XCDS
    tail = w >= n_whole
    k = np.where(tail, (w - n_whole) // max(r, 1), 0)
    item = np.where(tail, n_whole + (w - n_whole) - k * r, w)
    ranges = np.array([[chunk_range(cstart[t], kk, K) for kk in range(K)] for t in range(n_tile)], np.int64)    # [tile][k][cb, ce]
    cb = np.where(tail, ranges[item % n_tile, k, 0], 0)
    ce = np.where(tail, ranges[item % n_tile, k, 1], C)
    idle = tail & (cb >= ce)
    return dict(grid=grid, xcd=xcd, item=item, chunk=k, cb=cb, ce=ce, idle=idle, cut=tail,
                flag=np.where(tail, xcd * nx + item, -1), wait=np.where(~idle & (cb > 0), cb, -1),
                post=np.where(~idle & (ce < C), ce, -1), final=~idle & (ce == C), row=xcd * nx + item)
