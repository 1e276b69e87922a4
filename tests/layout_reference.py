"""An independent interpreter of the finalized predict layout, for the tests.

``export_plan`` takes the layout the library would upload for a model -- the planning stages of ``hibag_model.hip`` run on
the host through ``hibag_hip_test_layout_plan`` -- and ``audit`` reads it back the way the kernels do: it is written from
the layout's description in ``hibag_amd/csrc/hibag_device.h`` and from the reference's loop nest (src/LibHLA.cpp:1776-1821:
cells h1 <= h2, then i1 ascending, then i2, the diagonal pair (i, i) first on diagonal cells), not from the code that
builds the layout.  Findings come back as ``(rule, message)``; the rules are

  A.engine  A.hap                                   engines, operand rows; the haplotype table
  B.order  B.pad  B.pfac  B.phdr  B.store  B.blk_close  B.wide      the pass-1 lists
  C.slots  C.cstart  C.ehdr  C.ctile                the E-stream of pass 2
  D.tiles  D.cells                                  every cell evaluated or read from one stored row, never both
  E.stream  E.cls_cnt  E.tile_meta  E.items         the vector engine's records, the cell lists, the work items
  F.parow                                           the prebuilt A-operand rows
  G.bounds                                          every index a kernel forms, with the extent of its access
  H.replay                                          (``replay``: the posterior from the lists, in float64, slot order)

Plain numpy; the slot walks are vectorised (the largest test model has about a million slots)."""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

NA_INTEGER = -2147483648
END, STORE = 0x80000000, 0x40000000
CHUNK = 4
FP4, I8, I8S, VALU = 1, 2, 3, 0
STEP_SNPS, FP4_MAX_SNPS, MAX_STEPS = 28, 30, 4
# e2m1 codes 0..7 are the numbers 0, 0.5, 1, 1.5, 2, 3, 4, 6
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])

_INT32 = {"n_snp_c", "nwp", "snp_off", "snp_index", "snp_weight", "mask_row", "c_order", "tile_p0", "tile_n", "cls_off", "cls_n",
          "engine", "n_step", "bt_row", "cls_nblk", "item_split", "split_row", "split_cls", "item_whole", "cell_row", "wide_cls",
          "wide_seg", "wide_scan"}
_FLOAT = {"pfac", "split_heavy_ns", "split_rest_ns"}
_U64 = {"stream_off", "blk_off", "etile_blk0", "wide_seg_off"}


@dataclass
class Settings:
    """The overrides a model is laid out under (read from the environment by the library)."""
    pass2: str = "auto"          # HIBAG_PASS2: auto | stream | hybrid | recompute
    store_pairs: int = 12        # HIBAG_STORE_PAIRS
    prebuilt_mb: float = 128.0   # HIBAG_PREBUILT_MB
    engine: str = ""             # HIBAG_ENGINE: "" | valu | i8

    @classmethod
    def from_env(cls, env=os.environ):
        p = env.get("HIBAG_PASS2", "")
        sp = env.get("HIBAG_STORE_PAIRS")
        mb = env.get("HIBAG_PREBUILT_MB")
        return cls(p if p in ("stream", "hybrid", "recompute") else "auto", 12 if sp is None else max(0, int(sp or 0)),
                   128.0 if mb is None else float(mb), env.get("HIBAG_ENGINE", ""))


class Plan(dict):
    """name -> numpy array (a copy); scalars are ``int`` / ``float``.  ``tab`` is the model's mutation table."""

    def copy(self):
        return Plan({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.items()})


def new_model_handle(obj):
    """An unfinalized library model of ``obj`` (the caller frees it with hibag_hip_model_free)."""
    from hibag_amd import _lib
    L = _lib.lib()
    h = L.hibag_hip_model_new(int(obj.n_hla), int(obj.n_snp))
    if not h:
        raise _lib.HibagHipError(-1, L.hibag_hip_last_error().decode())
    h = C.c_void_p(h)
    for c in obj.classifiers:
        strs = (C.c_char_p * len(c.haplo))(*[s.encode() for s in c.haplo])
        idx = np.ascontiguousarray(c.snpidx, np.int32); fr = np.ascontiguousarray(c.freq, np.float64)
        hla = np.ascontiguousarray(c.hla, np.int32)
        _lib.check(L.hibag_hip_model_add_classifier(h, len(idx), idx.ctypes.data_as(C.c_void_p), len(fr),
                                                    fr.ctypes.data_as(C.c_void_p), hla.ctypes.data_as(C.c_void_p), strs))
    return h


def plan_of_handle(h) -> Plan:
    from hibag_amd import _lib
    L = _lib.lib()
    p = L.hibag_hip_test_layout_plan(h)
    if not p:
        raise _lib.HibagHipError(-1, L.hibag_hip_last_error().decode())
    p = C.c_void_p(p)
    out = Plan()
    try:
        for i in range(L.hibag_hip_test_layout_count(p)):
            name, data, nbytes, elem = C.c_char_p(), C.c_void_p(), C.c_uint64(), C.c_int()
            _lib.check(L.hibag_hip_test_layout_get(p, i, C.byref(name), C.byref(data), C.byref(nbytes), C.byref(elem)))
            key = name.value.decode()
            dt = (np.float64 if key in _FLOAT else np.uint64 if key in _U64 else np.int64) if elem.value == 8 else \
                 (np.int32 if key in _INT32 else np.uint32)
            raw = C.string_at(data.value, nbytes.value) if nbytes.value else b""
            a = np.frombuffer(raw, dt).copy()
            scalar = key.startswith("room:") or (elem.value == 8 and key not in _U64 and key != "pfac")
            out[key] = (float(a[0]) if key in _FLOAT else int(a[0])) if scalar else a
    finally:
        L.hibag_hip_test_layout_free(p)
    tab = np.empty(257, np.float64)
    _lib.check(L.hibag_hip_model_mutation_table(h, tab.ctypes.data_as(C.c_void_p)))
    out["tab"] = tab
    return out


def export_plan(obj) -> Plan:
    from hibag_amd import _lib
    h = new_model_handle(obj)
    try:
        return plan_of_handle(h)
    finally:
        _lib.lib().hibag_hip_model_free(h)


# ---------------------------------------------------------------------------------------------------------------------
# the model as the reference sees it

@dataclass
class Cls:
    H: int
    k: int
    freq: np.ndarray
    bits: np.ndarray          # [H, k] uint8
    st: np.ndarray            # [n_hla + 1] first haplotype of every allele
    snpidx: np.ndarray
    npairs: np.ndarray = None     # [P]
    cells: np.ndarray = None      # posterior indices of the non-empty cells
    seq: dict = field(default_factory=dict)


class Model:
    def __init__(self, obj):
        self.nh = nh = int(obj.n_hla)
        self.S = int(obj.n_snp)
        self.P = nh * (nh + 1) // 2
        h1 = np.repeat(np.arange(nh), np.arange(nh, 0, -1))
        first = np.concatenate([[0], np.cumsum(np.arange(nh, 0, -1))])[:-1]
        self.cell_h1 = h1
        self.cell_h2 = np.arange(self.P) - first[h1] + h1
        self.cls = []
        for c in obj.classifiers:
            H, k = len(c.freq), len(c.snpidx)
            bits = np.array([[ch == "1" for ch in s] for s in c.haplo], np.uint8).reshape(H, k)
            st = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(c.hla, np.int64), minlength=nh))]).astype(np.int64)
            k_ = Cls(H, k, np.asarray(c.freq, np.float64), bits, st, np.asarray(c.snpidx, np.int64))
            n1 = (st[1:] - st[:-1])[self.cell_h1]; n2 = (st[1:] - st[:-1])[self.cell_h2]
            k_.npairs = np.where(self.cell_h1 == self.cell_h2, n1 * (n1 + 1) // 2, n1 * n2)
            k_.cells = np.nonzero(k_.npairs)[0]
            self.cls.append(k_)
        self.C = len(self.cls)
        w = np.zeros(max(self.S, 1), np.int64)
        for k_ in self.cls:
            np.add.at(w, k_.snpidx, 1)
        self.snp_weight = w

    def pairs_of(self, c, cells):
        """The reference's visiting order of the haplotype pairs of `cells` (posterior indices, all non-empty) of classifier
        c, concatenated: (i1, i2, diag, factor, start offsets).  factor = f1 * f1 for the leading diagonal pair (i, i) of a
        diagonal cell (src/LibHLA.cpp:1786), (2 f1) * f2 otherwise (:1789-1793, :1808-1812)."""
        k = self.cls[c]
        cells = np.asarray(cells, np.int64)
        n = k.npairs[cells]
        start = np.concatenate([[0], np.cumsum(n)])
        ci = np.repeat(np.arange(len(cells)), n)
        r = np.arange(start[-1]) - start[ci]
        h1, h2 = self.cell_h1[cells][ci], self.cell_h2[cells][ci]
        a0, b0 = k.st[h1], k.st[h2]
        n1, n2 = k.st[h1 + 1] - a0, k.st[h2 + 1] - b0
        off = h1 != h2
        i1 = np.zeros(len(r), np.int64); i2 = np.zeros(len(r), np.int64); diag = np.zeros(len(r), bool)
        i1[off] = a0[off] + r[off] // np.maximum(n2[off], 1)
        i2[off] = b0[off] + r[off] % np.maximum(n2[off], 1)
        d = ~off
        if d.any():
            # row j of the triangle holds (j, j), (j, j + 1) ... : n1 - j pairs, the rows before it j n1 - j (j - 1) / 2
            m, rr = n1[d], r[d]
            j = np.floor(((2 * m + 1) - np.sqrt((2 * m + 1.0) ** 2 - 8.0 * rr)) / 2).astype(np.int64)
            before = lambda j: j * m - j * (j - 1) // 2
            j = np.where(before(j) > rr, j - 1, j)
            j = np.where(before(j + 1) <= rr, j + 1, j)
            assert np.all((before(j) <= rr) & (rr < before(j + 1)))
            col = rr - before(j)
            i1[d] = a0[d] + j; i2[d] = a0[d] + j + col; diag[d] = col == 0
        f = k.freq
        fac = np.where(diag, f[i1] * f[i1], (2 * f[i1]) * f[i2]) if len(r) else np.zeros(0)
        return i1, i2, diag, fac, start

    def slot_words(self, c, cells):
        """The slot words and factors of `cells` as the matrix engine lists them: the pairs in the reference's order,
        i1 | i2 << 16 with the leading diagonal pair as (H + 1 + i, i), each cell padded to an even slot count with the
        zero entry H, END on the cell's last slot.  Returns (words, factors, first slot of every cell (+ total))."""
        k = self.cls[c]
        i1, i2, diag, fac, start = self.pairs_of(c, cells)
        n = np.diff(start)
        ne = n + (n & 1)
        estart = np.concatenate([[0], np.cumsum(ne)])
        words = np.full(estart[-1], k.H | (k.H << 16), np.int64)
        facs = np.zeros(estart[-1])
        ci = np.repeat(np.arange(len(n)), n)
        dst = estart[ci] + (np.arange(start[-1]) - start[ci])
        words[dst] = np.where(diag, k.H + 1 + i1, i1) | (i2 << 16)
        facs[dst] = fac
        if len(n):
            words[estart[1:] - 1] |= END
        return words, facs, estart


def expected_engine(S: Settings, k: int, H: int):
    use_mfma, use_fp4 = S.engine != "valu", S.engine != "i8"
    if not (use_mfma and H < 16384):
        e = VALU
    elif use_fp4 and k <= FP4_MAX_SNPS:
        e = FP4
    elif k < 32:
        e = I8
    elif k == 32:
        e = I8S
    elif use_fp4 and k <= STEP_SNPS * MAX_STEPS:
        e = FP4
    else:
        e = VALU
    if e == FP4 and k > FP4_MAX_SNPS and S.pass2 == "recompute":
        e = VALU
    steps = 1 if e != FP4 or k <= FP4_MAX_SNPS else (k + STEP_SNPS - 1) // STEP_SNPS
    rows = 2 * steps if e == FP4 else 0 if e == VALU else 4
    return e, steps, rows


def round_nwp(n):
    for v in (1, 2, 3, 4, 6, 8, 10, 12):
        if n <= v:
            return v
    return 12


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _fields(lo, hi=None, n=8):
    """4-bit fields of 32-bit words (lo, hi) as [..., n]."""
    v = lo.astype(np.uint64) | ((hi.astype(np.uint64) << np.uint64(32)) if hi is not None else np.uint64(0))
    return ((v[..., None] >> (np.uint64(4) * np.arange(n, dtype=np.uint64))) & np.uint64(15)).astype(np.int64)


class Audit:
    def __init__(self, plan: Plan, model: Model, settings: Settings):
        self.L, self.M, self.S = plan, model, settings
        self.findings = []

    def fail(self, rule, msg):
        if len(self.findings) < 200:
            self.findings.append((rule, msg))

    def check(self, ok, rule, msg):
        if not ok:
            self.fail(rule, msg)
        return bool(ok)

    def rules(self):
        return {r for r, _ in self.findings}

    # -----------------------------------------------------------------------------------------------------------------
    def run(self):
        L = self.L
        self.C = self.M.C
        self.T = int(L["tile"]); self.NS = int(L["stored_per_visit"])
        if not self.check(L["n_classifier"] == self.C and L["n_hla"] == self.M.nh and L["n_cell"] == self.M.P, "A.engine", "model dimensions"):
            return self
        self.engine = L["engine"][:self.C].astype(np.int64); self.steps = L["n_step"][:self.C].astype(np.int64)
        self.rule_A_engine()
        self.rule_D_tiles()
        if "D.tiles" in self.rules() or "A.engine" in self.rules():
            return self                      # (everything below indexes by them)
        self.store_rule()
        self.rule_A_hap()
        self.rule_B()
        self.rule_C()
        self.rule_D()
        self.rule_E()
        self.rule_F()
        self.rule_G()
        return self

    def evaluates(self, c):
        return self.engine[c] == FP4 and self.steps[c] == 1

    def entry_dwords(self, c):
        return 12 if self.steps[c] == 1 else 8 + 4 * (int(self.steps[c]) - 1)

    # ---- A ---------------------------------------------------------------------------------------------------------
    def rule_A_engine(self):
        L, M = self.L, self.M
        row = 0
        for c, k in enumerate(M.cls):
            e, steps, rows = expected_engine(self.S, k.k, k.H)
            self.check(L["engine"][c] == e and L["n_step"][c] == steps, "A.engine", f"classifier {c}: engine {L['engine'][c]} x {L['n_step'][c]}, expected {e} x {steps}")
            self.check(L["bt_row"][c] == row, "A.engine", f"classifier {c}: bt_row {L['bt_row'][c]}, expected {row}")
            self.check(L["n_snp_c"][c] == k.k and L["nwp"][c] == round_nwp((3 * k.k + 31) // 32), "A.engine", f"classifier {c}: n_snp_c / nwp")
            row += rows
        self.check(L["bt_rows"] == row, "A.engine", f"bt_rows {L['bt_rows']}, expected {row}")
        self.check(L["bt_rows_alloc"] == max(row, 1) + 2, "A.engine", "bt_rows_alloc is not the model's rows and two spare")
        self.check(L["n_valu"] == int(np.sum(self.engine == VALU)), "A.engine", "n_valu")
        self.check(L["all_fp4"] == int(all(self.engine[c] == FP4 for c in range(self.C) if self.steps[c] == 1)), "A.engine", "all_fp4")
        self.check(np.array_equal(L["snp_weight"][:M.S], M.snp_weight[:M.S]), "A.engine", "snp_weight")
        self.check(L["pair_evals"] == sum(k.H * (k.H + 1) // 2 for k in M.cls), "A.engine", "pair_evals")

    def decode_hap(self, c):
        """The table of matrix-engine classifier c as (bits [2H + 1, k], ff [2H + 1], f [2H + 1], raw entries), or None."""
        L, k = self.L, self.M.cls[c]
        ed, n = self.entry_dwords(c), 2 * k.H + 1
        off = int(L["hap_off"][c])
        if off + n * ed > len(L["hap"]):
            self.fail("A.hap", f"classifier {c}: the table [{off}, {off + n * ed}) passes the end of hap ({len(L['hap'])})")
            return None
        ent = L["hap"][off:off + n * ed].reshape(n, ed)
        e, steps = self.engine[c], int(self.steps[c])
        nimg = 8 if steps == 1 else 4
        ffw = np.ascontiguousarray(ent[:, nimg:nimg + 4]).view(np.float64)
        bits = np.zeros((n, max(k.k, 1)), np.uint8)
        nib = lambda w: ((w[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(len(w), -1)     # [n, 8 * dwords]
        ok = True
        if e == FP4 and steps == 1:
            s_img, p_img = nib(ent[:, 0:4]), nib(ent[:, 4:8])
            real = np.arange(n) != k.H
            es, ep = np.zeros((n, 32), np.int64), np.zeros((n, 32), np.int64)
            hb = np.zeros((n, 32), np.int64)
            hb[:k.H, :k.k] = k.bits; hb[k.H + 1:, :k.k] = k.bits
            es += 2 * hb; ep += 3 * hb
            # the constants at nibbles k, k + 1 (not on the padding entry): sum image codes 1 and 3, pair image 3 and 3
            es[real, k.k] += 1; es[real, k.k + 1] += 3; ep[real, k.k] += 3; ep[real, k.k + 1] += 3
            ok = np.array_equal(s_img, es) and np.array_equal(p_img, ep)
            bits[:, :k.k] = (s_img[:, :k.k] == 2)
        elif e == FP4:
            img = np.concatenate([nib(ent[:, 0:4])[:, :STEP_SNPS]] + [nib(ent[:, 8 + 4 * j:12 + 4 * j])[:, :STEP_SNPS] for j in range(steps - 1)], 1)
            full = np.concatenate([nib(ent[:, 0:4])] + [nib(ent[:, 8 + 4 * j:12 + 4 * j]) for j in range(steps - 1)], 1)
            hb = np.zeros((n, STEP_SNPS * steps), np.int64)
            hb[:k.H, :k.k] = k.bits; hb[k.H + 1:, :k.k] = k.bits
            ok = np.array_equal(img, 2 * hb) and full.sum() == img.sum()          # (code 2 where the bit is set, nothing else anywhere)
            bits[:, :k.k] = (img[:, :k.k] == 2)
        else:
            by = ((ent[:, 0:8, None] >> (8 * np.arange(4, dtype=np.uint32))) & 255).reshape(n, 32)
            hb = np.zeros((n, 32), np.int64)
            hb[:k.H, :k.k] = k.bits; hb[k.H + 1:, :k.k] = k.bits
            ok = np.array_equal(by, hb)
            bits[:, :k.k] = by[:, :k.k] == 1
        self.check(ok, "A.hap", f"classifier {c}: the images of the table do not encode the haplotypes' bits")
        ff, f = ffw[:, 0], ffw[:, 1]
        want_f = np.concatenate([k.freq, [0.0], k.freq]); want_ff = np.concatenate([2 * k.freq, [0.0], k.freq])
        self.check(same_bits(f, want_f) and same_bits(ff, want_ff), "A.hap", f"classifier {c}: the table's {{ff, f}} are not {{2f, f}}, zero, {{f, f}}")
        return bits[:, :k.k], ff, f

    def rule_A_hap(self):
        L = self.L
        self.hap = {}
        at = 0
        for c in range(self.C):
            if self.engine[c] == VALU:
                continue
            self.check(L["hap_off"][c] == at, "A.hap", f"classifier {c}: hap_off {L['hap_off'][c]}, the tables before it end at {at}")
            self.hap[c] = self.decode_hap(c)
            at = int(L["hap_off"][c]) + (2 * self.M.cls[c].H + 1) * self.entry_dwords(c)
        # behind the tables: an all-zero one-step entry, the whole padded to 16 bytes; hap_dwords is the array's size
        self.check(L["hap_dwords"] == len(L["hap"]) and len(L["hap"]) % 4 == 0 and len(L["hap"]) >= at + 12 and not L["hap"][at:].any(),
                   "A.hap", "hap_dwords / the zero entry behind the tables")

    # ---- D (tiles), the store rule -----------------------------------------------------------------------------------
    def rule_D_tiles(self):
        L, M = self.L, self.M
        p0, n = L["tile_p0"].astype(np.int64), L["tile_n"].astype(np.int64)
        nt = int(L["n_tile"])
        ok = nt == len(p0) == len(n) and nt >= 1 and p0[0] == 0 and np.all(n >= 1) and np.all(n <= self.T) and \
            np.array_equal(p0[1:], (p0 + n)[:-1]) and p0[-1] + n[-1] == M.P
        if self.check(ok, "D.tiles", "the tiles do not cut the cells into consecutive runs of 1 .. HIBAG_TILE"):
            self.tile_p0, self.tile_n, self.n_tile = p0, n, nt
            self.tile_of = np.repeat(np.arange(nt), n)

    def store_rule(self):
        """Which cell sums pass 1 stores, recomputed from the comment above plan_store and DESIGN.md: mode 1 = every
        non-empty cell; mode 2 = every non-empty cell of a classifier pass 2 cannot evaluate, and of the others per (classifier,
        tile) the largest cells first, at most HIBAG_STORED_PER_VISIT: a cell of more than HIBAG_STORE_PAIRS pairs, or -- while the
        visit's remaining slots do not fit one block -- of at least five."""
        M, S = self.M, self.S
        recompute = S.pass2 == "recompute"
        above = float("inf") if recompute else S.store_pairs
        fit_min = float("inf") if recompute else 5
        ev = [self.evaluates(c) for c in range(self.C)]
        cost = sum(float(k.H * (k.H + 1) // 2) * (1.0 if self.engine[c] else 5.0) for c, k in enumerate(M.cls))
        n_cells = sum(len(k.cells) for k in M.cls)
        n_big = sum(int(np.sum(k.npairs > above)) if ev[c] else len(k.cells) for c, k in enumerate(M.cls))
        mode = 0 if self.C == 0 else 1 if cost >= 14.0 * max(n_cells, 1) else 2 if n_big else 0
        if S.pass2 == "stream":
            mode = int(self.C > 0)
        elif S.pass2 != "auto":
            mode = 2 if n_big else 0
        if mode == 2 and not any(ev):
            mode = 1
        self.mode = mode
        self.stored = []
        for c, k in enumerate(M.cls):
            st = np.zeros(M.P, bool)
            if mode == 1 or (mode == 2 and not ev[c]):
                st[k.cells] = True
            elif mode == 2:
                tiles = self.tile_of[k.cells]
                for t in np.unique(tiles):
                    cells = k.cells[tiles == t]
                    n = k.npairs[cells]
                    slots = int(np.sum(n + (n & 1)))
                    order = np.argsort(-n, kind="stable")
                    for i in order[:self.NS]:
                        if not (n[i] > above or (slots > 32 and n[i] >= fit_min)):
                            break
                        st[cells[i]] = True
                        slots -= int(n[i] + (n[i] & 1))
            self.stored.append(st)
        self.check(self.L["store_cells"] == mode, "B.store", f"store mode {self.L['store_cells']}, the rule gives {mode}")
        self.store_mode = int(self.L["store_cells"])

    # ---- B ---------------------------------------------------------------------------------------------------------
    def rule_B(self):
        L, M = self.L, self.M
        plist, pfac = L["plist"], L["pfac"]
        self.p1 = {}
        nblk_all = len(plist) // 32
        self.check(len(plist) % 32 == 0 and len(pfac) == len(plist) and len(L["phdr"]) == nblk_all * 4 and L["plist_dwords"] == len(plist),
                   "G.bounds", "plist, pfac and phdr do not have one size (or plist_dwords is not it)")
        # the headers follow from the words and factors, everywhere: {ends, stores, n_valid, 0}
        nb = min(nblk_all, len(pfac) // 32, len(L["phdr"]) // 4)
        w = plist[:nb * 32].reshape(nb, 32).astype(np.int64); fz = pfac[:nb * 32].reshape(nb, 32)
        sh = np.arange(32)
        ends = ((w >> 31) & 1); stores = (w >= (END | STORE)).astype(np.int64)
        live = (fz != 0) | (ends != 0)
        n_valid = np.where(live.any(1), 32 - np.argmax(live[:, ::-1], 1), 0)
        hdr = L["phdr"][:nb * 4].reshape(nb, 4).astype(np.int64)
        bad = np.nonzero((hdr[:, 0] != (ends << sh).sum(1)) | (hdr[:, 1] != (stores << sh).sum(1)) | (hdr[:, 2] != n_valid) | (hdr[:, 3] != 0))[0]
        self.check(len(bad) == 0, "B.phdr", f"{len(bad)} block headers do not follow from their slots, the first block {bad[:1]}")
        beyond = (sh[None, :] >= hdr[:, 2:3]) & live
        self.check(not beyond.any(), "B.phdr", "a slot with a factor or an END lies at or beyond n_valid")
        self.check(not np.any(((w >> 30) & 1) & ~((w >> 31) & 1)), "B.store", "STORE without END")
        self.ends_all, self.nvalid_all = (ends << sh).sum(1), n_valid

        at = int(L["p1_base"])
        self.check(at == int(L["estream_blocks"]) * 32, "B.order", "the pass-1 lists do not begin behind the E-stream")
        close_at = 0
        seg_i = 0
        wseg = L["wide_seg"].reshape(-1, 4) if int(L["n_wide_seg"]) else np.zeros((0, 4), np.int64)
        wide_cls, wide_scan, p1_blocks = [], [], 0
        for c, k in enumerate(M.cls):
            if self.engine[c] == VALU:
                continue
            nblk, off = int(L["cls_nblk"][c]), int(L["blk_off"][c])
            self.check(off == at, "B.order", f"classifier {c}: its list begins at {off}, the lists before it end at {at}")
            if off + nblk * 32 > len(plist):
                self.fail("G.bounds", f"classifier {c}: its list passes the end of plist")
                return
            words = plist[off:off + nblk * 32].astype(np.int64); facs = pfac[off:off + nblk * 32]
            pad = k.H | (k.H << 16)
            trailing = words == pad
            exp_w, exp_f, estart = M.slot_words(c, k.cells)
            wide = self.steps[c] > 1
            # segments: one for a one-step classifier; whole cells, each starting a block, for several K steps
            if wide:
                wide_cls.append(c)
                segs = []
                while seg_i < len(wseg) and wseg[seg_i][0] == c:
                    segs.append((int(L["wide_seg_off"][seg_i]), *[int(v) for v in wseg[seg_i][1:]]))
                    seg_i += 1
                whole = len(wide_cls_all(self)) >= 8
                pos = off
                for so, row, snb, flag in segs:
                    self.check(so == pos and snb > 0, "B.wide", f"classifier {c}: a segment at {so}, the one before ends at {pos}")
                    self.check(flag == int(whole), "B.wide", f"classifier {c}: the whole-classifier flag of a segment")
                    pos = so + snb * 32
                self.check(pos == off + nblk * 32, "B.wide", f"classifier {c}: the segments do not cover the list")
                if not (len(segs) == 1 and segs[0][3] == 1):
                    wide_scan.append(c)
                bounds = [(so - off) // 32 for so, *_ in segs] + [nblk]
            else:
                bounds = [0, nblk] if nblk else [0]
                segs = []
            # trailing padding: the zero entry without END, from behind an END to the end of a segment's last block
            real = np.nonzero(~trailing)[0]
            seg_ends = set(b * 32 for b in bounds[1:])
            ok_pad = True
            if trailing.any():
                tr = np.nonzero(trailing)[0]
                run_end = tr[np.nonzero(np.diff(np.concatenate([tr, [-5]])) != 1)[0]] + 1
                run_start = tr[np.nonzero(np.diff(np.concatenate([[-5], tr])) != 1)[0]]
                ok_pad = all(int(e) in seg_ends for e in run_end) and all(s > 0 and (words[s - 1] >> 31) & 1 for s in run_start) \
                    and all(e - s < 32 for s, e in zip(run_start, run_end))
            endpos = np.nonzero((words >> 31) & 1)[0]
            self.check(ok_pad and not np.any(endpos % 2 == 0), "B.pad", f"classifier {c}: an END on an even slot, or padding that is not the unused tail of a block")
            self.check(nblk == sum((int(np.sum(~trailing[a * 32:b * 32])) + 31) // 32 for a, b in zip(bounds[:-1], bounds[1:])) if nblk else len(exp_w) == 0,
                       "B.pad", f"classifier {c}: more blocks than its slots need")
            got = words[real] & ~STORE
            same = len(got) == len(exp_w) and np.array_equal(got, exp_w)
            self.check(same, "B.order", f"classifier {c}: the slots between the END flags are not the reference's pairs, cell after cell" +
                       ("" if same else f" (first difference at real slot {int(np.argmax(got != exp_w))})" if len(got) == len(exp_w) else f" ({len(got)} slots, {len(exp_w)} expected)"))
            if wide and same:
                # a segment holds whole cells and names the number of non-empty cells before it
                cum_end = np.concatenate([[0], np.cumsum((words >> 31) & 1)])
                for (so, row, snb, flag) in segs:
                    a = so - off
                    self.check(row == cum_end[a] and (a == 0 or trailing[a - 1] or (words[a - 1] >> 31) & 1), "B.wide",
                               f"classifier {c}: a segment's first stored row {row}, {cum_end[a]} cells close before it")
            fexp = np.zeros(len(words)); fexp[real[:len(exp_f)]] = exp_f[:len(real)]
            self.check(same_bits(facs, fexp), "B.pfac", f"classifier {c}: a slot's factor is not the reference's rounded product (+0.0 on padding)" +
                       (f", first at slot {int(np.argmax(facs.view(np.uint64) != fexp.view(np.uint64)))}" if len(facs) == len(fexp) and len(facs) else ""))
            # STORE exactly on the cells the rule stores
            if same:
                cell_end = real[estart[1:] - 1] if len(k.cells) else np.zeros(0, np.int64)
                flagged = ((words[cell_end] >> 30) & 1).astype(bool)
                want = self.stored[c][k.cells] if (self.store_mode or wide) else np.zeros(len(k.cells), bool)
                self.check(np.array_equal(flagged, want), "B.store", f"classifier {c}: STORE on {int(flagged.sum())} cells, the rule stores {int(want.sum())}" +
                           (f", first difference at cell {int(k.cells[np.argmax(flagged != want)])}" if len(flagged) == len(want) and len(want) else ""))
                self.p1[c] = dict(off=off, nblk=nblk, words=words, facs=facs, real=real, estart=estart, flagged=flagged, bounds=bounds)
            if self.store_mode:
                st = ((words >> 30) & 1).reshape(nblk, 32).sum(1) if nblk else np.zeros(0, np.int64)
                want = np.zeros(nblk, np.int64) if wide else np.concatenate([[0], np.cumsum(st)])[:nblk]
                got_c = L["blk_close"][close_at:close_at + nblk]
                self.check((off - int(L["p1_base"])) // 32 == close_at and np.array_equal(got_c, want), "B.blk_close",
                           f"classifier {c}: blk_close is not the number of stored cells closed in its earlier blocks")
                close_at += nblk
            at = off + nblk * 32
            p1_blocks += nblk
        self.p1_end = at
        self.check(L["p1_blocks"] == p1_blocks, "B.blk_close", "p1_blocks")
        self.check(len(L["blk_close"]) == (max(close_at, 1) if self.store_mode else 1), "B.blk_close", "blk_close has entries for other than the pass-1 blocks")
        self.check(seg_i == len(wseg) and L["n_wide_seg"] == len(wseg), "B.wide", "segments that belong to no classifier of several K steps, or out of order")
        self.check(list(L["wide_cls"][:L["n_wide"]]) == wide_cls and list(L["wide_scan"][:L["n_wide_scan"]]) == wide_scan, "B.wide",
                   "wide_cls / wide_scan do not name the classifiers of several K steps / those that are not one whole segment")
        # behind the lists: four blocks of slack, all zero
        self.check(len(plist) == at + 4 * 32 and not plist[at:].any() and not pfac[at:].any(), "G.bounds", "the four zero blocks of look-ahead slack behind the pass-1 lists")

    # ---- C ---------------------------------------------------------------------------------------------------------
    def rule_C(self):
        L, M, C, nt = self.L, self.M, self.C, self.n_tile
        eb = int(L["estream_blocks"])
        self.es = None
        cs = L["etile_cstart"].astype(np.int64)
        if not self.check(len(cs) == nt * (C + 1) and len(L["etile_blk0"]) == max(nt, 1) and len(L["ehdr"]) == eb * 8, "G.bounds", "etile_cstart / etile_blk0 / ehdr sizes"):
            return
        cs = cs.reshape(nt, C + 1)
        blk0 = L["etile_blk0"].astype(np.int64)
        if self.store_mode == 1 or C == 0:
            self.check(eb == 4 and not cs.any() and not blk0.any() and not L["ehdr"].any() and not L["plist"][:eb * 32].any(), "C.slots", "mode 1 has no E-stream but its slack")
            self.check_ctile(None)
            return
        # what every (tile, classifier) visit holds
        nvb = np.zeros((nt, C), np.int64); nbs = np.zeros((nt, C), np.int64)
        ev_list, st_list = [], []           # rows (t, c, p, j[, n slots])
        for c, k in enumerate(M.cls):
            t = self.tile_of[k.cells]
            stc = self.stored[c][k.cells] if self.store_mode == 2 else np.zeros(len(k.cells), bool)
            j = k.cells - self.tile_p0[t]
            if self.evaluates(c):
                n = k.npairs[k.cells]
                ne = (n + (n & 1)) * ~stc
                np.add.at(nbs[:, c], t, ne)
                e = ~stc
                ev_list.append(np.stack([t[e], np.full(e.sum(), c), k.cells[e], j[e], ne[e]], 1))
            else:
                self.check(stc.all(), "B.store", f"classifier {c} is not evaluated by pass 2 and has cells that are not stored")
            st_list.append(np.stack([t[stc], np.full(stc.sum(), c), k.cells[stc], j[stc]], 1))
            ns = np.bincount(t[stc], minlength=nt)
            nbs[:, c] = (nbs[:, c] + 31) // 32
            nvb[:, c] = np.maximum(nbs[:, c], (ns + self.NS - 1) // self.NS)
        want_cs = np.concatenate([np.zeros((nt, 1), np.int64), np.cumsum(nvb, 1)], 1)
        want_b0 = np.concatenate([[0], np.cumsum(want_cs[:, C])])
        ok = self.check(np.array_equal(cs, want_cs), "C.cstart", "etile_cstart: a classifier's blocks do not begin where the blocks of the classifiers before it end" +
                        (f" (first at tile, classifier {np.argwhere(cs != want_cs)[0]})" if cs.shape == want_cs.shape and (cs != want_cs).any() else ""))
        ok &= self.check(np.array_equal(blk0, want_b0[:nt]) and eb == want_b0[nt] + 4, "C.cstart", "etile_blk0 / estream_blocks: the tiles' blocks do not follow each other (+ 4 of slack)")
        if not ok or eb * 32 > len(L["plist"]):
            return
        nreal = int(want_b0[nt])
        vfirst = want_b0[:nt, None] + want_cs[:, :C]              # first block of every visit
        # the expected slots: per visit the evaluated cells' words, its last slot block filled up with the classifier's zero
        # entry; blocks that only carry stored sums, and the slack, are zero words
        exp = np.zeros(eb * 32, np.int64); expf = np.zeros(eb * 32)
        blk_c = np.repeat(np.tile(np.arange(C), nt), nvb.reshape(-1)); blk_t = np.repeat(np.repeat(np.arange(nt), C), nvb.reshape(-1))
        blk_i = np.arange(nreal) - np.repeat(vfirst.reshape(-1), nvb.reshape(-1))          # block's number inside its visit
        padw = np.array([k.H | (k.H << 16) for k in M.cls], np.int64)
        has_slots = blk_i < nbs[blk_t, blk_c]
        exp[:nreal * 32] = np.repeat(np.where(has_slots, padw[blk_c], 0), 32)
        end_rows = []
        for c, k in enumerate(M.cls):
            if not self.evaluates(c):
                continue
            rows = ev_list.pop(0)
            if not len(rows):
                continue
            w, f, estart = M.slot_words(c, rows[:, 2])
            t = rows[:, 0]
            # offset of every cell inside its visit: the slots of the visit's cells before it
            cum = np.cumsum(rows[:, 4]) - rows[:, 4]
            first_of_t = np.concatenate([[True], t[1:] != t[:-1]])
            base = np.maximum.accumulate(np.where(first_of_t, cum, 0))
            dst0 = vfirst[t, c] * 32 + (cum - base)
            ci = np.repeat(np.arange(len(rows)), rows[:, 4])
            dst = dst0[ci] + (np.arange(len(w)) - estart[ci])
            exp[dst] = w; expf[dst] = f
            end_rows.append(np.stack([dst0 + rows[:, 4] - 1, rows[:, 3]], 1))
        got = L["plist"][:eb * 32].astype(np.int64)
        same = np.array_equal(got, exp)
        self.check(same, "C.slots", "the E-stream's slots are not the reference's pairs of every tile's evaluated cells" +
                   (f" (first difference at slot {int(np.argmax(got != exp))})" if not same else ""))
        self.check(same_bits(L["pfac"][:eb * 32], expf), "B.pfac", "E-stream: a slot's factor is not the reference's rounded product")
        # ---- headers
        hd = L["ehdr"].reshape(eb, 8).astype(np.int64)
        ends = np.zeros(eb, np.int64); groups = np.zeros(eb, np.int64)
        ew = exp.reshape(eb, 32)
        ends = (((ew >> 31) & 1) << np.arange(32)).sum(1)
        live = (expf.reshape(eb, 32) != 0) | ((ew >> 31) & 1).astype(bool)
        nv = np.where(live.any(1), 32 - np.argmax(live[:, ::-1], 1), 0)
        groups = (nv + 3) // 4
        self.check(np.array_equal(hd[:, 0], ends), "C.ehdr", "word 0 is not the block's end mask")
        self.check(np.array_equal(hd[:, 6] >> 28, groups), "C.ehdr", "word 6: the count of four-slot groups worth evaluating")
        # bit 29: the last record gone through of the nearest block before that has any closed a cell
        last_end = np.where(groups > 0, (ends >> np.maximum(4 * groups - 1, 0)) & 1, 0)
        idx = np.maximum.accumulate(np.where(groups > 0, np.arange(eb), -1))
        prev = np.concatenate([[-1], idx[:-1]])
        fresh = np.where(prev >= 0, last_end[np.maximum(prev, 0)], 0)
        self.check(np.array_equal((hd[:, 1] >> 29) & 1, fresh), "C.ehdr", "word 1 bit 29: whether the record before the block's first one closed a cell" +
                   (f" (first at block {int(np.argmax(((hd[:, 1] >> 29) & 1) != fresh))})" if not np.array_equal((hd[:, 1] >> 29) & 1, fresh) else ""))
        self.check(not np.any(hd[:, 1] >> 30), "C.ehdr", "word 1: bits above 29")
        # words 4, 5: the tile row of each closing cell at field slot / 2
        jq = np.zeros((eb, 16), np.int64)
        if end_rows:
            er = np.concatenate(end_rows)
            jq[er[:, 0] // 32, (er[:, 0] % 32) // 2] = er[:, 1]
        self.check(np.array_equal(_fields(L["ehdr"].reshape(eb, 8)[:, 4], L["ehdr"].reshape(eb, 8)[:, 5], 16), jq), "C.ehdr",
                   "words 4, 5: the tile rows of the cells that close in the block")
        # stored sums: per visit its stored cells in cell order, HIBAG_STORED_PER_VISIT per block, rows counted on from the
        # classifier's first row and the stored cells of its earlier tiles
        srows = np.concatenate(st_list) if st_list else np.zeros((0, 4), np.int64)
        order = np.lexsort((srows[:, 2], srows[:, 0], srows[:, 1]))             # classifier, tile, cell
        srows = srows[order]
        cell_row = L["cell_row"].astype(np.int64)
        rank_c = np.arange(len(srows)) - np.searchsorted(srows[:, 1], srows[:, 1])      # position among the classifier's stored cells
        key = srows[:, 1] * nt + srows[:, 0]
        rank_v = np.arange(len(srows)) - np.searchsorted(key, key)
        sblk = vfirst[srows[:, 0], srows[:, 1]] + rank_v // self.NS
        cnt = np.bincount(sblk, minlength=eb)
        self.check(np.array_equal((hd[:, 1] >> 25) & 15, cnt), "C.ehdr", "word 1: the block's stored count" +
                   (f" (first at block {int(np.argmax(((hd[:, 1] >> 25) & 15) != cnt))})" if not np.array_equal((hd[:, 1] >> 25) & 15, cnt) else ""))
        first_row = np.zeros(eb, np.int64)
        sel = rank_v % self.NS == 0
        first_row[sblk[sel]] = cell_row[srows[sel, 1]] + rank_c[sel]
        has = cnt > 0
        self.check(np.array_equal((hd[:, 1] & 0x1FFFFFF)[has], first_row[has]), "C.ehdr", "word 1: the first stored row of the block's stored sums")
        jps = np.zeros((eb, 7), np.int64)
        jps[sblk, rank_v % self.NS] = srows[:, 3]
        self.check(np.array_equal(_fields(L["ehdr"].reshape(eb, 8)[:, 6], None, 7), jps), "C.ehdr", "word 6: the tile rows of the stored sums")
        # word 7: classifier | first operand row << 16 (a classifier without rows of its own: row 0); words 2, 3: the next block's 7 and 1
        bt = np.array([int(L["bt_row"][c]) if self.engine[c] != VALU else 0 for c in range(C)], np.int64)
        w7 = np.zeros(eb, np.int64)
        w7[:nreal] = blk_c | (bt[blk_c] << 16)
        self.check(np.array_equal(hd[:, 7], w7), "C.ehdr", "word 7 is not classifier | first operand row << 16" +
                   (f" (first at block {int(np.argmax(hd[:, 7] != w7))})" if not np.array_equal(hd[:, 7], w7) else ""))
        self.check(np.array_equal(hd[:-1, 2], hd[1:, 7]) and np.array_equal(hd[:-1, 3], hd[1:, 1]) and hd[-1, 2] == 0 and hd[-1, 3] == 0,
                   "C.ehdr", "words 2, 3 are not copies of the next block's words 7 and 1")
        self.es = dict(nreal=nreal, blk_c=blk_c, blk_t=blk_t, has_slots=has_slots)
        self.check_ctile((nvb, st_list))

    def check_ctile(self, _):
        L, M, C, nt = self.L, self.M, self.C, self.n_tile
        ct = L["ctile"]
        if not self.check(len(ct) == max(C, 1) * nt * 8 + 8, "G.bounds", "ctile size"):
            return
        ct = ct[:C * nt * 8].reshape(C, nt, 8).astype(np.int64)
        cell_row = L["cell_row"].astype(np.int64)
        for c, k in enumerate(M.cls):
            t = self.tile_of[k.cells]; j = k.cells - self.tile_p0[t]
            big = self.stored[c][k.cells] if self.store_mode == 2 else np.zeros(len(k.cells), bool)
            nlist = np.bincount(t[~big], minlength=nt); nst = np.bincount(t[big], minlength=nt)
            k_last = k.k - STEP_SNPS * (int(self.steps[c]) - 1)
            w0 = int(self.engine[c]) | ((k_last << 2) & 0xFC) | (nlist << 8) | ((int(self.steps[c]) - 1) << 13) | (int(L["bt_row"][c]) << 16)
            self.check(np.array_equal(ct[c, :, 0], w0), "C.ctile", f"classifier {c}: word 0 (engine, k of the last step, listed cells, steps - 1, bt_row)")
            self.check(np.all(ct[c, :, 1] == int(L["hap_off"][c])) and not ct[c, :, 2:5].any(), "C.ctile", f"classifier {c}: word 1 is not hap_off (or words 2-4 not zero)")
            per_tile = nst if self.store_mode == 2 else np.bincount(t, minlength=nt)
            k0 = np.cumsum(per_tile) - per_tile
            self.check(np.array_equal(ct[c, :, 5], (cell_row[c] + k0) | (nst << 27)), "C.ctile", f"classifier {c}: word 5 (first stored row | stored cells << 27)")
            # row list: listed cells in closing (= cell) order, then the stored ones
            order = np.lexsort((k.cells, big, t))
            tt = t[order]
            pos = np.arange(len(tt)) - np.searchsorted(tt, tt)
            jp = np.zeros((nt, 16), np.int64)
            jp[tt, pos] = j[order]
            self.check(np.array_equal(_fields(L["ctile"][:C * nt * 8].reshape(C, nt, 8)[c, :, 6], L["ctile"][:C * nt * 8].reshape(C, nt, 8)[c, :, 7], 16), jp),
                       "C.ctile", f"classifier {c}: the row list")
        spp = sum(int(k.npairs[k.cells][~(self.stored[c][k.cells] if self.store_mode == 2 else np.zeros(len(k.cells), bool))].sum())
                  for c, k in enumerate(M.cls) if self.evaluates(c)) if self.store_mode != 1 else 0
        self.check(L["second_pass_pairs"] == spp, "C.ctile", f"second_pass_pairs {L['second_pass_pairs']}, the evaluated cells hold {spp}")

    # ---- D ---------------------------------------------------------------------------------------------------------
    def pass1_rows(self):
        """row -> (classifier, cell) as pass 1 writes them: the k-th STORE-flagged cell of a matrix-engine classifier goes to row
        cell_row[c] + k (k_total's `row`, k_total_wide from wide_seg[1]); a vector-engine classifier that stores writes row i for
        its i-th non-empty cell (classifier_total)."""
        L, M = self.L, self.M
        cell_row = L["cell_row"].astype(np.int64)
        out = {}
        split = set(int(c) for c in L["split_cls"][:L["n_split"]])
        for c, k in enumerate(M.cls):
            if self.engine[c] == VALU:
                cells = k.cells if (self.store_mode or c in split) else k.cells[:0]
            elif c in self.p1:
                cells = k.cells[self.p1[c]["flagged"]]
            else:
                continue
            out[c] = (cell_row[c] + np.arange(len(cells)), cells)
        return out

    def rule_D(self):
        L, M, C = self.L, self.M, self.C
        cell_row = L["cell_row"].astype(np.int64)
        if not self.check(len(cell_row) == C + 1 and cell_row[0] == 0 and np.all(np.diff(cell_row) >= 0) and L["cell_rows"] == cell_row[C], "D.cells", "cell_row"):
            return
        split = set(int(c) for c in L["split_cls"][:L["n_split"]])
        w1 = self.pass1_rows()
        for c, k in enumerate(M.cls):
            want = len(k.cells) if (self.store_mode == 1 or c in split) else int(self.stored[c].sum()) if self.store_mode == 2 else 0
            self.check(cell_row[c + 1] - cell_row[c] == want, "D.cells", f"classifier {c} has {cell_row[c + 1] - cell_row[c]} rows, {want} stored cells")
            if c in w1:
                self.check(len(w1[c][0]) == 0 or w1[c][0][-1] < cell_row[c + 1], "D.cells", f"classifier {c}: pass 1 writes beyond its rows")
        owner = np.full((max(int(cell_row[C]), 1), 2), -1, np.int64)
        evaluated = [np.zeros(M.P, np.int64) for _ in range(C)]; read = [np.zeros(M.P, np.int64) for _ in range(C)]
        if self.store_mode == 1:
            ct = L["ctile"][:C * self.n_tile * 8].reshape(C, self.n_tile, 8).astype(np.int64)
            for c in range(C):
                n = (ct[c, :, 0] >> 8) & 31; row = ct[c, :, 5] & 0x7FFFFFF
                jl = _fields(L["ctile"][:C * self.n_tile * 8].reshape(C, self.n_tile, 8)[c, :, 6], L["ctile"][:C * self.n_tile * 8].reshape(C, self.n_tile, 8)[c, :, 7], 16)
                for t in np.nonzero(n)[0]:
                    for i in range(int(n[t])):
                        self.note_read(owner, read, c, int(self.tile_p0[t] + jl[t, i]), int(row[t] + i), cell_row)
        elif self.es is not None:
            eb = int(L["estream_blocks"]); nreal = self.es["nreal"]
            hd = L["ehdr"].reshape(eb, 8)
            cc = (hd[:nreal, 7] & 0xFFFF).astype(np.int64); tt = self.es["blk_t"]
            cnt = ((hd[:nreal, 1] >> 25) & 15).astype(np.int64); row = (hd[:nreal, 1] & 0x1FFFFFF).astype(np.int64)
            js = _fields(hd[:nreal, 6], None, 7)
            for b in np.nonzero(cnt)[0]:
                for i in range(int(cnt[b])):
                    if cc[b] < C:
                        self.note_read(owner, read, int(cc[b]), int(self.tile_p0[tt[b]] + js[b, i]), int(row[b] + i), cell_row)
            jq = _fields(hd[:nreal, 4], hd[:nreal, 5], 16)
            endbits = ((hd[:nreal, 0:1].astype(np.int64) >> (2 * np.arange(16) + 1)) & 1).astype(bool)
            bb, ff = np.nonzero(endbits)
            ok = cc[bb] < C
            p = self.tile_p0[tt[bb]] + jq[bb, ff]
            for c in np.unique(cc[bb][ok]):
                pc = p[ok & (cc[bb] == c)]
                pc = pc[pc < M.P]
                np.add.at(evaluated[c], pc, 1)
        for c, k in enumerate(M.cls):
            tot = evaluated[c] + read[c]
            want = (k.npairs > 0).astype(np.int64)
            bad = np.nonzero(tot != want)[0]
            self.check(len(bad) == 0, "D.cells", f"classifier {c}: {len(bad)} cells are not evaluated or read exactly once in pass 2, the first cell {bad[:1]} "
                       f"(evaluated {evaluated[c][bad[:1]]}, read {read[c][bad[:1]]})")
            # what pass 2 reads is what pass 1 wrote there
            if c in w1:
                rows, cells = w1[c]
                rd = np.nonzero(read[c])[0]
                got = {int(p): int(r) for r, (cc_, p) in enumerate(owner) if cc_ == c}
                self.check(all(got.get(int(p)) == int(r) for r, p in zip(rows, cells) if read[c][p]) and set(rd) <= set(int(p) for p in cells), "D.cells",
                           f"classifier {c}: pass 2 reads a row pass 1 does not write that cell's sum to")

    def note_read(self, owner, read, c, p, row, cell_row):
        if not (cell_row[c] <= row < cell_row[c + 1]) or not (0 <= p < self.M.P):
            self.fail("D.cells", f"classifier {c}: stored row {row} is not one of its rows [{cell_row[c]}, {cell_row[c + 1]})")
            return
        if owner[row][0] >= 0:
            self.fail("D.cells", f"row {row} serves two cells")
        owner[row] = (c, p)
        read[c][p] += 1

    # ---- E ---------------------------------------------------------------------------------------------------------
    def rule_E(self):
        L, M, C, nt = self.L, self.M, self.C, self.n_tile
        cnt_all, cell_all = L["cls_cnt"].astype(np.int64), L["cls_cell"].astype(np.int64)
        at, s_at = 0, 0
        tm = L["tile_meta"]
        self.check(len(tm) == max(C, 1) * nt * (4 + self.T) + 1, "G.bounds", "tile_meta size")
        self.valu = {}
        for c, k in enumerate(M.cls):
            chunks = (k.npairs[k.cells] + CHUNK - 1) // CHUNK
            n = len(k.cells)
            ok = L["cls_off"][c] == at and L["cls_n"][c] == n and at + n + 1 <= len(cnt_all) and np.array_equal(cnt_all[at:at + n], chunks) and \
                np.array_equal(cell_all[at:at + n], k.cells) and cnt_all[at + n] == 0 and cell_all[at + n] == 0
            self.check(ok, "E.cls_cnt", f"classifier {c}: cls_cnt / cls_cell are not the chunk counts and cells of its non-empty cells (+ a zero)")
            at += n + 1
            # tile_meta[c][t] = {#non-empty, first chunk, rows packed (2 dwords), (j << 24 | chunks) non-empty then empty}
            if len(tm) >= (c + 1) * nt * (4 + self.T):
                me = tm[c * nt * (4 + self.T):(c + 1) * nt * (4 + self.T)].reshape(nt, 4 + self.T).astype(np.int64)
                t = self.tile_of[k.cells]; j = k.cells - self.tile_p0[t]
                per = np.bincount(t, minlength=nt)
                cht = np.bincount(t, weights=chunks, minlength=nt).astype(np.int64)
                want = np.zeros((nt, 4 + self.T), np.int64)
                want[:, 0] = per; want[:, 1] = np.cumsum(cht) - cht
                pos = np.arange(n) - np.searchsorted(t, t)
                jp = np.zeros(nt, np.int64)
                np.add.at(jp, t, j << (4 * pos))
                want[:, 2] = jp & 0xFFFFFFFF; want[:, 3] = jp >> 32
                want[t, 4 + pos] = (j << 24) | chunks
                full = np.zeros(M.P, bool); full[k.cells] = True
                emp = np.nonzero(~full)[0]
                te = self.tile_of[emp]
                pe = np.arange(len(emp)) - np.searchsorted(te, te) + per[te]
                want[te, 4 + pe] = (emp - self.tile_p0[te]) << 24
                self.check(np.array_equal(me, want), "E.tile_meta", f"classifier {c}: tile_meta")
            if self.engine[c] != VALU:
                continue
            nwp, off = int(L["nwp"][c]), int(L["stream_off"][c])
            cd = CHUNK * (nwp + 2)
            T = int(chunks.sum())
            self.check(off % 2 == 0 and off >= s_at, "E.stream", f"classifier {c}: stream_off")
            if off + T * cd > len(L["stream"]):
                self.fail("G.bounds", f"classifier {c}: its records pass the end of stream")
                continue
            s_at = off + T * cd
            raw = L["stream"][off:off + T * cd].reshape(T, cd)
            W = raw[:, :nwp * CHUNK].reshape(T, nwp, CHUNK).transpose(0, 2, 1).reshape(T * CHUNK, nwp)
            prod = np.ascontiguousarray(raw[:, nwp * CHUNK:]).view(np.float64).reshape(T * CHUNK)
            i1, i2, diag, fac, start = M.pairs_of(c, k.cells)
            cstart = np.concatenate([[0], np.cumsum(chunks * CHUNK)])
            ci = np.repeat(np.arange(n), np.diff(start))
            dst = cstart[ci] + (np.arange(start[-1]) - start[ci])
            eprod = np.zeros(T * CHUNK); eprod[dst] = fac
            b1, b2 = k.bits[i1], k.bits[i2]
            bits = np.zeros((len(i1), nwp * 32), np.uint8)
            bits[:, :k.k] = b1; bits[:, k.k:2 * k.k] = b2; bits[:, 2 * k.k:3 * k.k] = 1 - (b1 ^ b2)
            eW = np.zeros((T * CHUNK, nwp), np.uint32)
            if len(i1):
                eW[dst] = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(len(i1), nwp)
            self.check(np.array_equal(W, eW) and same_bits(prod, eprod), "E.stream", f"classifier {c}: the records are not the reference's pair sequence "
                       "(W = H1 | H2 << k | ~(H1 ^ H2) << 2k, prod, cells in whole chunks, padding {0, +0.0})")
            self.valu[c] = dict(i1=i1, i2=i2, prod=prod, dst=dst, cstart=cstart, W=W)
        self.check(len(cnt_all) == max(at, 1), "E.cls_cnt", "cls_cnt has entries behind the last classifier's")
        self.check(L["stream_bytes"] == 4 * len(L["stream"]), "E.stream", "stream_bytes")
        # work items: {classifier, first cell, end cell, first chunk} in the classifier's non-empty list
        narrow = [c for c in range(C) if self.steps[c] == 1]
        iw = L["item_whole"].reshape(-1, 4)[:L["n_item_whole"]].astype(np.int64)
        ok = sorted(iw[:, 0].tolist()) == narrow and all(r[1] == 0 and r[2] == len(M.cls[r[0]].cells) and r[3] == 0 for r in iw if r[0] < C)
        self.check(ok, "E.items", "item_whole does not cover every one-step classifier's cell list once")
        it = L["item_split"].reshape(-1, 4)[:L["n_item_split"]].astype(np.int64)
        split = []
        ok = set(it[:, 0].tolist()) == set(narrow)
        for c in narrow:
            r = it[it[:, 0] == c]
            r = r[np.argsort(r[:, 1], kind="stable")]
            ch = (M.cls[c].npairs[M.cls[c].cells] + CHUNK - 1) // CHUNK
            cum = np.concatenate([[0], np.cumsum(ch)])
            n = len(M.cls[c].cells)
            ok &= len(r) >= 1 and r[0, 1] == 0 and r[-1, 2] == n and np.array_equal(r[1:, 1], r[:-1, 2]) and \
                (len(r) == 1 or bool(np.all(r[:, 2] > r[:, 1]))) and np.array_equal(r[:, 3], cum[np.minimum(r[:, 1], n)])
            if len(r) > 1:
                split.append(c)
        self.check(ok, "E.items", "item (the split list) does not cover every one-step classifier's cell list once in contiguous ranges with their first chunks")
        sc = [int(c) for c in L["split_cls"][:L["n_split"]]]
        sr = [c for c in range(C) if L["split_row"][c] >= 0]
        self.check(sc == sr and set(split) <= set(sc) and all(self.engine[c] == VALU for c in sc) and all(len(it[it[:, 0] == c]) > 1 for c in sc), "E.items",
                   "split_cls / split_row do not name exactly the classifiers whose cell list is cut")

    # ---- F ---------------------------------------------------------------------------------------------------------
    def rule_F(self):
        L, M = self.L, self.M
        pb = int(L["parow_blocks"]); nb_all = len(L["plist"]) // 32
        fp4_blocks = sum(int(L["cls_nblk"][c]) for c in range(self.C) if self.evaluates(c))
        pre = fp4_blocks > 0 and nb_all * 1024.0 <= self.S.prebuilt_mb * 1e6
        self.check(L["p1_prebuilt"] == int(pre) and pb == (nb_all if pre else int(L["estream_blocks"])) and len(L["parow"]) == pb * 256, "F.parow",
                   "p1_prebuilt / parow_blocks do not follow HIBAG_PREBUILT_MB")
        if len(L["parow"]) != pb * 256 or pb * 32 > len(L["plist"]):
            return
        # decoded e2m1 values, times two, of every lane row: [block, 64 lanes, 32 nibbles]
        val2 = (2 * E2M1).astype(np.uint8)
        words = L["plist"][:pb * 32].astype(np.int64)
        exp = np.zeros((pb * 32, 2, 32), np.uint8)
        ranges = []
        if self.es is not None:
            bc = self.es["blk_c"]
            for c in range(self.C):
                if self.evaluates(c):
                    blocks = np.nonzero((bc == c) & self.es["has_slots"])[0]       # (blocks that only carry stored sums: zero rows)
                    ranges.append((c, (blocks[:, None] * 32 + np.arange(32)).reshape(-1)))
        if pre:
            for c in range(self.C):
                if self.evaluates(c):
                    o, n = int(L["blk_off"][c]), int(L["cls_nblk"][c])
                    ranges.append((c, np.arange(o, o + n * 32)))
        for c, slots in ranges:
            if c not in self.hap or self.hap[c] is None or not len(slots):
                continue
            k = M.cls[c]
            hb = self.hap[c][0]
            w = words[slots]
            e1, e2 = w & 0xFFFF, (w >> 16) & 0x3FFF
            okm = (e1 <= 2 * k.H) & (e2 <= 2 * k.H)
            if not okm.all():
                self.fail("G.bounds", f"classifier {c}: a slot names a table entry beyond 2H")
                continue
            real = ~((e1 == k.H) & (e2 == k.H))
            ssum = hb[e1].astype(np.int64) + hb[e2]                       # S = h1 + h2 at [0, k)
            ex = np.zeros((len(slots), 2, 32), np.uint8)
            ex[:, 0, :k.k] = 2 * ssum                                     # the A column: S at [0, k) ...
            ex[:, 1, :k.k] = np.array([0, 3, 8], np.uint8)[ssum]          # ... w(S) = 0 / 1.5 / 4 at [32, 32 + k)
            half = real & ((e1 == k.H) | (e2 == k.H))                     # (no such slot in a correct list)
            if half.any():
                self.fail("F.parow", f"classifier {c}: a slot pairs a haplotype with the zero entry")
            ex[real, 0, k.k] = 2; ex[real, 0, k.k + 1] = 8                # 1, 4 at k, k + 1
            ex[real, 1, k.k] = 8; ex[real, 1, k.k + 1] = 8                # 4, 4 at 32 + k, 32 + k + 1
            exp[slots] = ex
        pr = L["parow"].reshape(pb, 64, 4)
        nib = ((pr[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).astype(np.uint8).reshape(pb, 64, 32)
        got = val2[nib].reshape(pb, 2, 32, 32).transpose(0, 2, 1, 3).reshape(pb * 32, 2, 32)      # lane = half * 32 + slot
        bad = np.nonzero((got != exp).any((1, 2)))[0]
        self.check(len(bad) == 0, "F.parow", f"{len(bad)} prebuilt rows are not the A column of their slot's pair, the first at slot {bad[:1]}")

    # ---- G ---------------------------------------------------------------------------------------------------------
    def rule_G(self):
        """Every index a kernel forms from a layout word, plus the extent of the access, against the exported size of the array
        (the table in DESIGN.md section 22 names the kernel lines)."""
        L, M, C, nt = self.L, self.M, self.C, self.n_tile
        g = lambda ok, msg: self.check(ok, "G.bounds", msg)
        nblk_plist = len(L["plist"]) // 32
        # the scalars the kernels build their buffer descriptors from describe arrays that exist
        g(L["plist_dwords"] <= len(L["plist"]) and L["plist_dwords"] <= len(L["pfac"]) and L["plist_dwords"] // 32 * 4 <= len(L["phdr"]),
          "plist_dwords exceeds plist / pfac / phdr")           # hibag_k_engine.h:461, :537 (descriptor of the list), :410-411
        g(L["hap_dwords"] <= len(L["hap"]), "hap_dwords exceeds hap")                                         # hibag_k_engine.h:595
        g(L["parow_blocks"] * 256 <= len(L["parow"]), "parow_blocks exceeds parow")                           # hibag_k_engine.h:414, hibag_k_pass2.h:105
        g(L["estream_blocks"] * 8 <= len(L["ehdr"]) and L["estream_blocks"] <= nblk_plist, "estream_blocks exceeds ehdr / plist")
        for name in ("n_snp_c", "nwp", "engine", "n_step", "bt_row", "cls_nblk", "hap_off", "cls_off", "cls_n", "split_row", "stream_off", "blk_off", "mask_row"):
            g(len(L[name]) >= C, f"{name} has fewer than C entries")
        g(len(L["cell_row"]) >= C + 1, "cell_row has fewer than C + 1 entries")                               # hibag_k_pass1.h:18
        g(len(L["tile_p0"]) >= nt and len(L["tile_n"]) >= nt, "tile_p0 / tile_n")
        for name in L:
            if name.startswith("room:"):
                a = L[name[5:]]
                g(L[name] >= a.nbytes, f"{name} is smaller than the array")
        cell_rows = int(L["cell_row"][C]) if len(L["cell_row"]) > C else 0
        alloc = int(L["bt_rows_alloc"])
        # -- table entries of a classifier's own slots: entry * size + 16 bytes of an image inside hap (hibag_k_engine.h:547-548,
        #    :572-573 one-step and int8; :481-485 several K steps: every step's image of the entry)
        for c, k in enumerate(M.cls):
            if self.engine[c] == VALU:
                continue
            ed = self.entry_dwords(c)
            g(int(L["hap_off"][c]) < L["hap_dwords"], f"classifier {c}: hap_off beyond hap_dwords")          # hibag_k_engine.h:595 (unsigned difference)
            o, n = int(L["blk_off"][c]), int(L["cls_nblk"][c])
            if o + n * 32 <= len(L["plist"]):
                w = L["plist"][o:o + n * 32].astype(np.int64)
                emax = max(int((w & 0xFFFF).max(initial=0)), int(((w >> 16) & 0x3FFF).max(initial=0)))
                g(int(L["hap_off"][c]) + (emax + 1) * ed <= L["hap_dwords"], f"classifier {c}: a slot's table entry {emax} passes the end of hap")
            # -- a walk of blocks [b0, b1) of the list (k_total: [0, cls_nblk) or a chunk of it, hibag_k_pass1.h:166-173, :225;
            #    k_total_wide: a segment, :291) reads the header of block b1 (hibag_k_engine.h:430, :499, :569), the first
            #    TOTAL_G = 8 factors of block b1 (:431, :500, :570), the slot words of blocks b1 and b1 + 1 through a descriptor
            #    that ends at plist_dwords (:543, :574, :478, :502) and, on prebuilt rows, the rows of block b1 through a
            #    descriptor that ends at parow_blocks (:438, :444)
            ends = [o // 32 + n] if self.steps[c] == 1 else []
            for e in ends:
                self.walk_extent(c, e)
            # -- blk_close[(blk_off[c] - p1_base) / 32 + b0], b0 < cls_nblk (hibag_k_pass1.h:198, STORE builds)
            if self.store_mode and n:
                g((o - int(L["p1_base"])) // 32 + n - 1 < len(L["blk_close"]) and (o - int(L["p1_base"])) // 32 + n <= L["p1_blocks"],
                  f"classifier {c}: its blocks' blk_close entries pass the end")
        # -- wide_seg[4 i ..], wide_seg_off[i] for i < n_wide_seg (hibag_k_pass1.h:273, :291)
        nseg = int(L["n_wide_seg"])
        g(len(L["wide_seg"]) >= 4 * nseg and len(L["wide_seg_off"]) >= nseg, "wide_seg / wide_seg_off shorter than n_wide_seg")
        for i in range(min(nseg, len(L["wide_seg_off"]), len(L["wide_seg"]) // 4)):
            so, (c, row, nb, _) = int(L["wide_seg_off"][i]), [int(v) for v in L["wide_seg"][4 * i:4 * i + 4]]
            g(so % 32 == 0 and 0 <= c < C, f"segment {i}: offset / classifier")
            if 0 <= c < C:
                self.walk_extent(c, so // 32 + nb)
                # (its rows: cell_rows(c) + row, one per cell that closes in the segment, hibag_k_pass1.h:281-284)
                if c in self.p1 and so + nb * 32 <= len(L["plist"]):
                    closes = int(np.sum((L["plist"][so:so + nb * 32] >> 31) & 1))
                    g(int(L["cell_row"][c]) + row + closes <= cell_rows, f"segment {i}: its stored rows pass cell_row[C]")
        # -- vector engine: classifier_total reads cls_cnt[cls_off[c] + i + 1] for i < cls_n (hibag_k_pass1.h:32) and the chunks
        #    [stream_off, + chunks * HIBAG_CHUNK_DWORDS(nwp)) (hibag_k_pass1.h:28, hibag_k_engine.h:49-58, :70)
        for c, k in enumerate(M.cls):
            g(int(L["cls_off"][c]) + int(L["cls_n"][c]) + 1 <= len(L["cls_cnt"]), f"classifier {c}: the one-ahead read of cls_cnt passes its end")
            if self.engine[c] == VALU:
                chunks = int(L["cls_cnt"][int(L["cls_off"][c]):int(L["cls_off"][c]) + int(L["cls_n"][c])].sum())
                cd = CHUNK * (int(L["nwp"][c]) + 2)
                g(int(L["stream_off"][c]) + chunks * cd <= len(L["stream"]), f"classifier {c}: its chunks pass the end of stream")
                # (the layout keeps one widest chunk of slack behind the last record; no read that needs it was found in the kernels)
                g(int(L["stream_off"][c]) + chunks * cd + CHUNK * 14 <= len(L["stream"]), f"classifier {c}: the documented chunk of slack behind stream")
        # -- work items (hibag_k_pass1.h:162-166, :239)
        for name, cnt in (("item_whole", "n_item_whole"), ("item_split", "n_item_split")):
            it = L[name][:4 * int(L[cnt])].reshape(-1, 4).astype(np.int64)
            g(len(L[name]) >= 4 * int(L[cnt]) and (not len(it) or (it[:, 0].min() >= 0 and it[:, 0].max() < C)), f"{name}: classifier out of range")
            if len(it) and it[:, 0].max() < C and it[:, 0].min() >= 0:
                g(bool(np.all((0 <= it[:, 1]) & (it[:, 1] <= it[:, 2]) & (it[:, 2] <= L["cls_n"][it[:, 0]]))), f"{name}: a cell range outside the classifier's list")
        g(all(0 <= int(c) < C for c in L["split_cls"][:L["n_split"]]) and all(0 <= int(c) < C for c in L["wide_scan"][:L["n_wide_scan"]]), "split_cls / wide_scan")
        # -- pass 2, k_accum_cells (mode 1): ctile[c][t] for all c, t (hibag_k_pass2.h:313); rows [word 5 & 0x7FFFFFF, + listed
        #    cells) of the group's cell_row[C] rows (:322-328); the row list's fields index HIBAG_TILE accumulator rows (:342)
        g(len(L["ctile"]) >= C * nt * 8, "ctile shorter than [C][n_tile][8]")
        if len(L["ctile"]) >= C * nt * 8 and C:
            ct = L["ctile"][:C * nt * 8].reshape(C, nt, 8).astype(np.int64)
            n = (ct[:, :, 0] >> 8) & 31
            if self.store_mode == 1:
                g(bool(np.all((ct[:, :, 5] & 0x7FFFFFF) + n <= cell_rows)), "ctile: a visit's stored rows pass cell_row[C]")
                jl = _fields(L["ctile"][:C * nt * 8].reshape(C, nt, 8)[:, :, 6], L["ctile"][:C * nt * 8].reshape(C, nt, 8)[:, :, 7], 16)
                used = np.arange(16)[None, None, :] < n[:, :, None]
                g(bool(np.all(jl[used] < self.T)) and bool(np.all(n <= self.T)), "ctile: a row-list field names a tile row beyond HIBAG_TILE")
            g(bool(np.all((ct[:, :, 0] >> 16) + 2 <= alloc)), "ctile: an operand row (and the one behind it) beyond the rows of the batch's array")
            g(bool(np.all(ct[:, :, 1] < max(int(L["hap_dwords"]), 1))), "ctile: hap_off beyond hap_dwords")
        # -- pass 2, k_accum (modes 0 and 2)
        if self.store_mode != 1 and len(L["etile_cstart"]) >= nt * (C + 1) and len(L["etile_blk0"]) >= nt:
            eb = int(L["estream_blocks"])
            cs = L["etile_cstart"][:nt * (C + 1)].reshape(nt, C + 1).astype(np.int64)
            be = L["etile_blk0"][:nt].astype(np.int64) + cs[:, C]            # one past the tile's last block
            g(bool(np.all(np.diff(cs, axis=1) >= 0)), "etile_cstart is not ascending")                       # hibag_k_pass2.h:96-97, chunk_bound
            # a walk of a tile's blocks [bb, be) reads the header of block be (hibag_k_pass2.h:179), the factors of block be up
            # to its dword 48 (:180, :186), and requests the rows of block be through a descriptor that ends at parow_blocks (:228)
            g(bool(np.all(be + 1 <= eb)) and (be.max(initial=0) + 1) * 8 <= len(L["ehdr"]), "a tile's walk reads a header beyond ehdr")
            g((be.max(initial=0) + 1) * 32 <= len(L["pfac"]), "a tile's walk reads factors beyond pfac")
            g(be.max(initial=0) <= L["parow_blocks"], "a tile's blocks have no prebuilt rows")
            # (the layout keeps four blocks of slack behind the E-stream; the reads above need one)
            g(be.max(initial=0) + 4 <= eb, "the four blocks of look-ahead slack behind the E-stream")
            if eb * 8 <= len(L["ehdr"]):
                hd = L["ehdr"][:eb * 8].reshape(eb, 8).astype(np.int64)
                for wi, what in ((7, "word 7"), (2, "word 2")):
                    # classifier -> its {weight, 1/total} row of C (hibag_k_pass2.h:155); operand rows r and r + 1 of the
                    # batch's bt_rows_alloc rows (:152-154)
                    g(bool(np.all((hd[:, wi] & 0xFFFF) < max(C, 1))), f"ehdr {what}: classifier beyond C")
                    bad = np.nonzero((hd[:, wi] >> 16) + 2 > alloc)[0]
                    g(len(bad) == 0, f"ehdr {what}: operand row {int((hd[bad[:1], wi] >> 16)[0]) if len(bad) else 0} and the one behind it pass the {alloc} rows of the batch's array (block {bad[:1]})")
                for wi in (1, 3):
                    # stored sums: rows [row, row + count) of cell_row[C] (hibag_k_pass2.h:137-145)
                    cnt = (hd[:, wi] >> 25) & 15
                    g(bool(np.all(cnt <= self.NS)) and bool(np.all(((hd[:, wi] & 0x1FFFFFF) + cnt)[cnt > 0] <= cell_rows)), f"ehdr word {wi}: stored rows beyond cell_row[C]")
                # tile rows index the HIBAG_TILE accumulator rows in LDS (hibag_k_pass2.h:204, :239-241)
                jq = _fields(L["ehdr"][:eb * 8].reshape(eb, 8)[:, 4], L["ehdr"][:eb * 8].reshape(eb, 8)[:, 5], 16)
                js = _fields(L["ehdr"][:eb * 8].reshape(eb, 8)[:, 6], None, 7)
                g(bool(np.all(jq < self.T)) and bool(np.all(js < self.T)), "ehdr words 4-6: a tile row beyond HIBAG_TILE")

    def walk_extent(self, c, e):
        """A pass-1 walk that ends with block e - 1 (absolute block number): what it reads behind it."""
        L = self.L
        g = lambda ok, msg: self.check(ok, "G.bounds", f"classifier {c}: a walk that ends at block {e} {msg}")
        g((e + 1) * 4 <= len(L["phdr"]), "reads a header beyond phdr")
        g(e * 32 + 8 <= len(L["pfac"]), "reads factors beyond pfac")
        g((e + 2) * 32 <= L["plist_dwords"], "requests slot words beyond plist_dwords")
        if L["p1_prebuilt"] and self.evaluates(c):
            g(e + 1 <= L["parow_blocks"], "requests prebuilt rows beyond parow_blocks")


def wide_cls_all(a: Audit):
    return [c for c in range(a.C) if a.steps[c] > 1]


def audit(plan: Plan, obj_or_model, settings: Settings) -> Audit:
    model = obj_or_model if isinstance(obj_or_model, Model) else Model(obj_or_model)
    return Audit(plan, model, settings).run()


# ---------------------------------------------------------------------------------------------------------------------
# H: the numeric replay

def _ordered_cell_sums(term, cell_id, n_cells):
    """sums[cell] = the terms of the cell added in slot order, one addition at a time (float64, no reassociation)."""
    out = np.zeros((n_cells, term.shape[1]))
    if not len(term):
        return out
    first = np.searchsorted(cell_id, np.arange(n_cells))
    pos = np.arange(len(cell_id)) - first[cell_id]
    order = np.argsort(pos, kind="stable")
    cut = np.searchsorted(pos[order], np.arange(int(pos.max()) + 2))
    for k in range(len(cut) - 1):
        sel = order[cut[k]:cut[k + 1]]
        out[cell_id[sel]] += term[sel]            # (a cell has one slot at each position: no index repeats)
    return out


def _distance(b1, b2, g):
    """[pairs, samples]: the distance of hibag_device.h per SNP -- g = 0: h1 + h2; g = 2: 2 - h1 - h2; g = 1: [h1 == h2];
    anything else (missing): 0 -- summed over the classifier's SNPs."""
    S = b1.astype(np.float32) + b2.astype(np.float32)
    m0, m1, m2 = (g == 0).T.astype(np.float32), (g == 1).T.astype(np.float32), (g == 2).T.astype(np.float32)
    d = S @ m0 + (2 - S) @ m2 + (b1 == b2).astype(np.float32) @ m1
    return d.astype(np.int64)


def replay(a: Audit, G):
    """The posterior [n_samp, P] from the layout alone, twice: from pass 1's lists, and as pass 2 sees it (the evaluated cells
    from the E-stream, the stored ones from pass 1's sums through their rows).  Needs a clean audit of rules A - E."""
    L, M, C = a.L, a.M, a.C
    G = np.asarray(G, np.int64)
    ns = len(G)
    tab = L["tab"]
    cell1 = np.zeros((C, M.P, ns)); cell2 = np.zeros((C, M.P, ns))
    rows = np.full((max(int(L["cell_row"][C]), 1), ns), np.nan)
    w1 = a.pass1_rows()
    for c, k in enumerate(M.cls):
        g = G[:, k.snpidx] if k.k else np.zeros((ns, 0), np.int64)
        if a.engine[c] == VALU:
            v = a.valu[c]
            W, prod = v["W"], v["prod"]
            bits = np.unpackbits(np.ascontiguousarray(W).view(np.uint8), axis=1, bitorder="little")
            term = prod[:, None] * tab[_distance(bits[:, :k.k], bits[:, k.k:2 * k.k], g)]
            cid = np.searchsorted(v["cstart"], np.arange(len(prod)), side="right") - 1
            sums = _ordered_cell_sums(term, cid, len(k.cells))
        else:
            p = a.p1[c]
            hb = a.hap[c][0]
            words, facs = p["words"], p["facs"]
            ends = (words >> 31) & 1
            cid = np.concatenate([[0], np.cumsum(ends)])[:-1]
            keep = cid < len(k.cells)                              # (the unused slots behind the last cell)
            e1, e2 = words[keep] & 0xFFFF, (words[keep] >> 16) & 0x3FFF
            term = facs[keep][:, None] * tab[_distance(hb[e1], hb[e2], g)]
            sums = _ordered_cell_sums(term, cid[keep], len(k.cells))
        cell1[c, k.cells] = sums
        if c in w1:
            r, cells = w1[c]
            pos = np.searchsorted(k.cells, cells)
            rows[r] = sums[pos]
    # pass 2's view
    if a.store_mode == 1:
        nt = a.n_tile
        ct = L["ctile"][:C * nt * 8].reshape(C, nt, 8)
        for c in range(C):
            n = ((ct[c, :, 0] >> 8) & 31).astype(np.int64); row = (ct[c, :, 5] & 0x7FFFFFF).astype(np.int64)
            jl = _fields(ct[c, :, 6], ct[c, :, 7], 16)
            for t in np.nonzero(n)[0]:
                cell2[c, a.tile_p0[t] + jl[t, :n[t]]] = rows[row[t]:row[t] + n[t]]
    elif a.es is not None:
        eb, nreal = int(L["estream_blocks"]), a.es["nreal"]
        hd = L["ehdr"].reshape(eb, 8)
        cc, tt = (hd[:nreal, 7] & 0xFFFF).astype(np.int64), a.es["blk_t"]
        cnt = ((hd[:nreal, 1] >> 25) & 15).astype(np.int64); row = (hd[:nreal, 1] & 0x1FFFFFF).astype(np.int64)
        js = _fields(hd[:nreal, 6], None, 7)
        for b in np.nonzero(cnt)[0]:
            cell2[cc[b], a.tile_p0[tt[b]] + js[b, :cnt[b]]] = rows[row[b]:row[b] + cnt[b]]
        jq = _fields(hd[:nreal, 4], hd[:nreal, 5], 16)
        for c, k in enumerate(M.cls):
            blocks = np.nonzero(cc == c)[0]
            if not a.evaluates(c) or not len(blocks):
                continue
            g = G[:, k.snpidx] if k.k else np.zeros((ns, 0), np.int64)
            slots = (blocks[:, None] * 32 + np.arange(32)).reshape(-1)
            words, facs = L["plist"][slots].astype(np.int64), L["pfac"][slots]
            ends = (words >> 31) & 1
            cid = np.concatenate([[0], np.cumsum(ends)])[:-1]
            ncell = int(ends.sum())
            keep = cid < ncell
            # (a block's unused tail sits between two cells of different visits: zero factors, they belong to no cell)
            pad = (words == (k.H | (k.H << 16)))
            keep &= ~pad
            hb = a.hap[c][0]
            e1, e2 = words[keep] & 0xFFFF, (words[keep] >> 16) & 0x3FFF
            term = facs[keep][:, None] * tab[_distance(hb[e1], hb[e2], g)]
            sums = _ordered_cell_sums(term, cid[keep], ncell)
            epos = slots[np.nonzero(ends)[0]]
            p = a.tile_p0[tt[epos // 32]] + jq[epos // 32, (epos % 32) // 2]
            cell2[c, p] = sums
    return _combine(M, cell1, G), _combine(M, cell2, G)


def _combine(M: Model, cell, G):
    """The ensemble step as the reference does it (src/LibHLA.cpp:1826-1828, :2418-2459, :1497-1518): in-order total of a
    classifier's cells, 1 / total, the classifier's weight from the sample's missing SNPs, the weighted sum over the
    classifiers in order, divided by the sum of weights."""
    ns = G.shape[0]
    post = np.zeros((M.P, ns)); sum_w = np.zeros(ns)
    with np.errstate(all="ignore"):
        for c, k in enumerate(M.cls):
            sw = M.snp_weight[k.snpidx]
            called = (G[:, k.snpidx] >= 0) & (G[:, k.snpidx] <= 2)
            tot, nw = int(sw.sum()), (called * sw).sum(1)
            w = nw / tot if tot > 0 else np.zeros(ns)
            use = w > 0
            total = np.zeros(ns)
            for p in range(M.P):
                total = total + cell[c, p]
            ff = 1 / total
            post[:, use] += ((cell[c] * ff) * w)[:, use]
            sum_w[use] += w[use]
        ok = sum_w > 0
        post[:, ok] *= (1.0 / sum_w[ok])
    return np.ascontiguousarray(post.T)
