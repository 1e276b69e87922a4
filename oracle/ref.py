"""ctypes front-end of ``oracle/_ref/libhibag_ref.so``: the HIBAG library sources themselves, compiled by
``oracle.build_ref()`` behind the C entries of ``ref_driver.cpp``.

TEST INFRASTRUCTURE ONLY.  This is what the oracle (``oracle.py``) is pinned against by execution
(``tests/test_ref_pin.py``) and the host that drives the plugin table on the device (``tests/test_hip_ref_host.py``).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import oracle as O

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")

TARGETS = ("base", "sse2", "sse4", "avx", "avx2")     # (the AVX-512 targets fuse multiply and add: not bit-comparable)


class RefError(RuntimeError):
    pass


_lib = None


def lib(path=None) -> C.CDLL:
    global _lib
    if _lib is None:
        L = C.CDLL(path or O.REF_LIB_PATH)
        L.ref_last_error.restype = C.c_char_p
        L.ref_cpu_info.restype = C.c_char_p
        L.ref_set_unif_rand.argtypes = [C.c_void_p, C.c_void_p]
        L.ref_set_target.argtypes = [C.c_char_p]
        L.ref_set_gpu_table.argtypes = [C.c_void_p, C.c_int]
        L.ref_model_new.restype = C.c_void_p
        L.ref_model_new.argtypes = [C.c_int] * 3
        L.ref_model_new_training.restype = C.c_void_p
        L.ref_model_new_training.argtypes = [C.c_int, C.c_int, _i32p, C.c_int, _i32p, _i32p]
        L.ref_model_free.argtypes = [C.c_void_p]
        L.ref_model_add_classifier.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_void_p, C.c_int, _f64p, _i32p,
                                               C.POINTER(C.c_char_p), C.c_double]
        L.ref_model_predict.argtypes = [C.c_void_p, _i32p, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.ref_model_train.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ref_model_n_classifier.argtypes = [C.c_void_p]
        L.ref_classifier_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.ref_classifier_get.argtypes = [C.c_void_p, C.c_int, _i32p, _i32p, _f64p, _i32p, _u64p]
        L.ref_match_info.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_longlong)] * 2
        L.ref_match_get.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _check(rc: int) -> int:
    if rc < 0:
        raise RefError(lib().ref_last_error().decode(errors="replace"))
    return rc


def set_target(name: str) -> str:
    """``CAlg_Prediction::Init_Target_IFunc(name)``; returns the library's CPU description."""
    _check(lib().ref_set_target(name.encode()))
    return lib().ref_cpu_info().decode()


def set_gpu_table(address, record: bool = False) -> None:
    """``HLA_LIB::GPUExtProcPtr`` = a copy of the ``TypeGPUExtProc`` at ``address`` (``None`` / 0 clears it).
    ``record``: keep every ``build_haplomatch`` call for :func:`match_calls`."""
    _check(lib().ref_set_gpu_table(C.c_void_p(address or None), int(record)))


def gpu_table_is_set() -> bool:
    return bool(lib().ref_gpu_table_is_set())


def reset() -> None:
    """The library's global state as at load: no plugin, no random source, the default target."""
    set_gpu_table(None)
    lib().ref_set_unif_rand(None, None)
    set_target("max")


class _Rng:
    """R's ``set.seed(seed)`` stream as the oracle restates it (``oracle_rng_set_seed`` / ``oracle_rng_unif``, pinned on
    printed values by tests/test_oracle_train.py), installed as the library's ``unif_rand``."""

    def __init__(self, seed: int):
        OL = O.lib()
        self.state = (C.c_uint32 * 626)()
        OL.oracle_rng_set_seed(self.state, C.c_uint(seed & 0xFFFFFFFF))
        fn = C.cast(OL.oracle_rng_unif, C.c_void_p)
        lib().ref_set_unif_rand(fn, C.cast(self.state, C.c_void_p))

    def close(self):
        lib().ref_set_unif_rand(None, None)


class Model:
    """One ``CAttrBag_Model`` of the compiled reference."""

    def __init__(self, handle, n_snp, n_samp, n_hla):
        if not handle:
            raise RefError(lib().ref_last_error().decode(errors="replace"))
        self.h, self.n_snp, self.n_samp, self.n_hla = C.c_void_p(handle), n_snp, n_samp, n_hla

    @classmethod
    def from_obj(cls, model, n_samp: int = 0):
        """Every classifier of an ``hlaAttrBagObj``-like object (see oracle.py) through ``Assign``."""
        self = cls(lib().ref_model_new(int(model.n_snp), int(n_samp), int(model.n_hla)), int(model.n_snp), int(n_samp),
                   int(model.n_hla))
        for c in model.classifiers:
            self.add_classifier(c.snpidx, c.freq, c.hla, c.haplo)
        return self

    @classmethod
    def for_training(cls, genomat, h1, h2, n_hla: int):
        g = np.ascontiguousarray(genomat, np.int32)
        n_samp, n_snp = g.shape
        a1, a2 = np.ascontiguousarray(h1, np.int32), np.ascontiguousarray(h2, np.int32)
        return cls(lib().ref_model_new_training(n_snp, n_samp, g.reshape(-1), int(n_hla), a1, a2), n_snp, n_samp, int(n_hla))

    def add_classifier(self, snpidx, freq, hla, haplo, acc: float = 0.0):
        ix = np.ascontiguousarray(snpidx, np.int32)
        f = np.ascontiguousarray(freq, np.float64)
        a = np.ascontiguousarray(hla, np.int32)
        strs = (C.c_char_p * max(len(f), 1))(*[s.encode() for s in haplo])
        one = np.zeros(1, np.int32)
        _check(lib().ref_model_add_classifier(self.h, len(ix), ix if len(ix) else one, None, len(f),
                                              f if len(f) else np.zeros(1), a if len(a) else one, strs, float(acc)))

    def predict(self, genomat, vote_method: int = 1):
        """``PredictHLA`` with all six outputs, keyed like ``oracle.predict``."""
        g = np.ascontiguousarray(genomat, np.int32)
        n, P = g.shape[0], self.n_hla * (self.n_hla + 1) // 2
        assert g.shape[1] == self.n_snp
        out = dict(h1=np.zeros(n, np.int32), h2=np.zeros(n, np.int32), prob=np.zeros(n, np.float64),
                   matching=np.zeros(n, np.float64), dosage=np.zeros((n, self.n_hla), np.float64),
                   postprob=np.zeros((n, P), np.float64))
        ptr = [out[k].ctypes.data_as(C.c_void_p) for k in ("h1", "h2", "prob", "matching", "dosage", "postprob")]
        _check(lib().ref_model_predict(self.h, g.reshape(-1), n, int(vote_method), *ptr))
        return out

    def train(self, nclassifier: int, mtry: int, prune: bool = True, seed: int = 100):
        """``set.seed(seed)`` + ``BuildClassifiers``; returns the classifiers in the form of ``oracle.train``, with the
        haplotype bits at or above each classifier's SNP count cleared (the library leaves them uninitialised)."""
        rng = _Rng(seed)
        try:
            n = _check(lib().ref_model_train(self.h, int(nclassifier), int(mtry), int(bool(prune))))
        finally:
            rng.close()
        return [self.classifier(i) for i in range(n)]

    def classifier(self, i: int):
        ns, nh, acc = C.c_int(0), C.c_int(0), C.c_double(0)
        _check(lib().ref_classifier_info(self.h, i, C.byref(ns), C.byref(nh), C.byref(acc)))
        k, H = ns.value, nh.value
        snpidx, samp = np.zeros(max(k, 1), np.int32), np.zeros(max(self.n_samp, 1), np.int32)
        freq, hla, bits = np.zeros(max(H, 1), np.float64), np.zeros(max(H, 1), np.int32), np.zeros(2 * max(H, 1), np.uint64)
        _check(lib().ref_classifier_get(self.h, i, snpidx, samp, freq, hla, bits))
        bits = bits.reshape(-1, 2)[:H] & low_mask(k)
        return dict(snpidx=snpidx[:k], samp_num=samp[:self.n_samp], freq=freq[:H], hla=hla[:H], bits=bits, acc=acc.value)

    def free(self):
        if self.h:
            lib().ref_model_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def low_mask(k: int) -> np.ndarray:
    """uint64 [2]: the low ``k`` of 128 bits."""
    m = (1 << k) - 1
    return np.array([m & 0xFFFFFFFFFFFFFFFF, m >> 64], np.uint64)


HAPLO_DT = np.dtype([("bits", "<u8", 2), ("freq", "<f8"), ("freq_f32", "<f4"), ("hla", "<i4")])
GENO_DT = np.dtype([("s1", "<u8", 2), ("s2", "<u8", 2), ("boot", "<i4"), ("a1", "<i4"), ("a2", "<i4"), ("pad", "<i4")])
assert HAPLO_DT.itemsize == 32 and GENO_DT.itemsize == 48


def match_calls():
    """The ``build_haplomatch`` calls recorded since ``set_gpu_table(..., record=True)``: dicts of haplo (HAPLO_DT),
    lens [n_hla], n_snp, geno (GENO_DT, every sample), out_n and buf (uint32, ``None`` for a NULL return)."""
    L = lib()
    out = []
    for i in range(L.ref_match_count()):
        nh, na, ns, ng = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        out_n, blen = C.c_longlong(0), C.c_longlong(0)
        _check(L.ref_match_info(i, C.byref(nh), C.byref(na), C.byref(ns), C.byref(ng), C.byref(out_n), C.byref(blen)))
        haplo, geno = np.zeros(max(nh.value, 1), HAPLO_DT), np.zeros(max(ng.value, 1), GENO_DT)
        lens, buf = np.zeros(max(na.value, 1), np.int64), np.zeros(max(blen.value, 1), np.uint32)
        _check(L.ref_match_get(i, haplo.ctypes.data, lens.ctypes.data, geno.ctypes.data, buf.ctypes.data))
        out.append(dict(haplo=haplo[:nh.value], lens=lens[:na.value], n_snp=ns.value, geno=geno[:ng.value],
                        out_n=out_n.value, buf=None if blen.value < 0 else buf[:blen.value]))
    return out
