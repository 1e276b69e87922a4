"""GPU parity of the training-side plugin entries (build_* of TypeGPUExtProc,
inst/include/LibHLA_ext.h:358-388), driven the way the reference's greedy SNP
search drives a plugin (src/LibHLA.cpp:1913-1979, :1002-1073):

* build_acc_oob against the `outofbag.acc` values the REFERENCE stored in its two
  bundled models (2 x 100 classifiers) -- known answers, not oracle outputs;
* build_acc_ib and build_haplomatch against the oracle's restatements of
  _PostProb / _PrepHaploMatch, bit for bit;
* the same three entries on CONSTRUCTED inputs at every SNP word count (tests/training_reference.py; their properties
  are checked by tests/test_training_inputs_host.py): no fixture classifier has more than 24 SNPs, so the fixtures run
  build_eval<1> and one turn of match_dist's word loop only.
"""

import ctypes as C
import math

import numpy as np
import pytest

import training_reference as T
from conftest import align_geno
from test_hip_parity import _TGenotype, _THaplotype

pytestmark = pytest.mark.gpu


class _FullTable(C.Structure):           # inst/include/LibHLA_ext.h:358-388
    _fields_ = [
        ("build_init", C.CFUNCTYPE(None, C.c_int, C.c_int)),
        ("build_done", C.CFUNCTYPE(None)),
        ("build_set_bootstrap", C.CFUNCTYPE(None, C.POINTER(C.c_int))),
        ("build_haplomatch", C.CFUNCTYPE(C.POINTER(C.c_uint32), C.POINTER(_THaplotype), C.POINTER(C.c_size_t), C.c_int,
                                         C.POINTER(_TGenotype), C.POINTER(C.c_size_t))),
        ("build_set_haplo_geno", C.CFUNCTYPE(None, C.POINTER(_THaplotype), C.c_int, C.POINTER(_TGenotype), C.c_int)),
        ("build_acc_oob", C.CFUNCTYPE(C.c_int)),
        ("build_acc_ib", C.CFUNCTYPE(C.c_double)),
        ("predict_init", C.c_void_p), ("predict_done", C.c_void_p), ("predict_avg_prob", C.c_void_p)]


def _i64(v):
    v = int(v)
    return v - (1 << 64) if v >> 63 else v


def _truth(model, table):
    ti = {s: i for i, s in enumerate(table["sample.id"])}
    lut = {a: i for i, a in enumerate(model.hla_allele)}
    return ([lut[table["A.1"][ti[s]]] for s in model.sample_id], [lut[table["A.2"][ti[s]]] for s in model.sample_id])


@pytest.mark.parametrize("which", ["oob", "a"])
def test_training_entries(which, oracle, hapmap_geno, hla_type_table, model_oob, model_a):
    import hibag_amd
    from hibag_amd import _lib
    hibag_amd.hlaSetKernelTarget("hip")
    model = model_oob if which == "oob" else model_a
    tab = _FullTable.from_address(_lib.lib().hibag_hip_gpu_ext_proc())
    fm = oracle.flatten(model)
    G = align_geno(model, hapmap_geno)
    a1, a2 = _truth(model, hla_type_table)
    n, nh = model.n_samp, model.n_hla
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]

    tab.build_init(nh, n)
    for c, cl in enumerate(model.classifiers):
        k, lens, bits, freq, _ = fm.classifier(c)
        H = len(freq)
        hap = (_THaplotype * H)()
        hla = np.repeat(np.arange(nh), lens)
        for i in range(H):
            hap[i].packed[0] = _i64(bits[i, 0]); hap[i].packed[1] = -1      # garbage above n_snp like the reference
            hap[i].freq = freq[i]; hap[i].freq_f32 = freq[i]; hap[i].hla = int(hla[i])
        geno = (_TGenotype * n)()
        planes = []
        for s in range(n):
            s1, s2 = oracle.int_to_snp(G[s], cl.snpidx)
            planes.append((s1, s2))
            for w in range(2):
                geno[s].s1[w] = _i64(s1[w]); geno[s].s2[w] = _i64(s2[w])
            geno[s].boot = int(cl.samp_num[s])
            geno[s].a1, geno[s].a2 = (a2[s], a1[s]) if s % 2 else (a1[s], a2[s])   # either order must work
        boot = (C.c_int * n)(*[int(v) for v in cl.samp_num])
        tab.build_set_bootstrap(boot)
        tab.build_set_haplo_geno(hap, H, geno, k)

        oob = np.where(cl.samp_num == 0)[0]
        inbag = np.where(cl.samp_num > 0)[0]
        # known answer stored by the reference: 0.5 * correct / nOOB (src/LibHLA.cpp:2121)
        assert tab.build_acc_oob() == round(cl.outofbag_acc * 2 * len(oob)), f"classifier {c}"

        if c % 10 == 0:                    # the oracle loops below are Python-slow; every 10th classifier
            loglik = 0.0
            for s in inbag:
                loglik += int(cl.samp_num[s]) * math.log(oracle.post_prob(fm, c, planes[s][0], planes[s][1], a1[s], a2[s]))
            assert tab.build_acc_ib() == -2 * loglik, f"classifier {c}"

            n_per = (C.c_size_t * nh)(*[int(v) for v in lens])
            out_n = C.c_size_t(0)
            buf = tab.build_haplomatch(hap, n_per, k, geno, C.byref(out_n))
            cnt = buf[0] // 2
            assert out_n.value == 1 + 2 * cnt
            got = {}
            for q in range(cnt):
                kk, v = buf[1 + 2 * q], buf[2 + 2 * q]
                got.setdefault(kk, []).append((v & 0xFFFF, v >> 16))
            libc.free(buf)
            st = np.concatenate([[0], np.cumsum(lens)])
            for kk, s in enumerate(inbag):
                lo, hi = sorted((a1[s], a2[s]))
                want = oracle.prep_haplo_match(fm, c, planes[s][0], planes[s][1], lo, hi)
                want = [(int(i) - int(st[lo]), int(j) - int(st[hi])) for i, j in want]
                assert got.get(kk, []) == want, f"classifier {c}, in-bag sample {kk}"
                assert len(want) >= 1            # the host insists on a non-empty list (src/LibHLA.cpp:1066-1072)
    tab.build_done()


class _Entries:
    """The plugin table over one constructed case (tests/training_reference.py), from build_init to build_done."""

    def __init__(self, cs):
        import hibag_amd
        from hibag_amd import _lib
        hibag_amd.hlaSetKernelTarget("hip")
        lst = cs.lst
        self.n, self.nh, self.k, self.H = len(cs.boot), lst.n_hla, lst.n_snp, len(lst.allele)
        self.tab = _FullTable.from_address(_lib.lib().hibag_hip_gpu_ext_proc())
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]
        self.hap_r, self.geno_r = lst.records(), cs.records()
        self.hap = C.cast(self.hap_r.ctypes.data, C.POINTER(_THaplotype))
        self.geno = C.cast(self.geno_r.ctypes.data, C.POINTER(_TGenotype))
        self.n_per = (C.c_size_t * self.nh)(*[int(v) for v in lst.lens])

    def __enter__(self):
        self.tab.build_init(self.nh, self.n)
        return self

    def __exit__(self, *exc):
        self.tab.build_done()

    def bootstrap(self, counts):
        self.tab.build_set_bootstrap((C.c_int * self.n)(*[int(v) for v in counts]))

    def scores(self):
        """build_set_haplo_geno, then (build_acc_oob, build_acc_ib)"""
        self.tab.build_set_haplo_geno(self.hap, self.H, self.geno, self.k)
        return self.tab.build_acc_oob(), self.tab.build_acc_ib()

    def haplomatch(self):
        """build_haplomatch's buffer, copied and freed, and its out_n"""
        out_n = C.c_size_t(0)
        buf = self.tab.build_haplomatch(self.hap, self.n_per, self.k, self.geno, C.byref(out_n))
        pairs = np.ctypeslib.as_array(buf, shape=(1 + buf[0],)).copy()
        self.libc.free(buf)
        return pairs, out_n.value


def _check_entries(key, cs, want, scores_again=False):
    """build_set_haplo_geno + build_acc_oob / build_acc_ib / build_haplomatch through the table on one constructed case,
    against the oracle, exactly.  ``scores_again``: the two scores once more after build_haplomatch."""
    with _Entries(cs) as e:
        e.bootstrap(cs.boot)
        got_oob, got_ib = e.scores()
        pairs, out_n = e.haplomatch()
        again = e.scores() if scores_again else None
    cnt = int(pairs[0]) // 2
    print(f"{key}: acc_oob {got_oob} (want {want.acc_oob}), acc_ib {got_ib!r} (want {want.loss_ib!r}), {cnt} pairs")
    assert got_oob == want.acc_oob
    assert got_ib == want.loss_ib
    assert out_n == 1 + 2 * cnt
    got = {}
    for q in range(cnt):
        kk, v = int(pairs[1 + 2 * q]), int(pairs[2 + 2 * q])
        got.setdefault(kk, []).append((v & 0xFFFF, v >> 16))
    refs = T.haplo_matches(cs)
    assert len(refs) == int((cs.boot > 0).sum())
    for kk, ref in enumerate(refs):
        assert got.get(kk, []) == ref, f"in-bag sample {kk}"
        assert len(ref) >= 1            # the host insists on a non-empty list (src/LibHLA.cpp:1066-1072)
    assert set(got) <= set(range(len(refs)))
    if scores_again:
        print(f"{key}: after build_haplomatch acc_oob {again[0]}, acc_ib {again[1]!r}")
        assert again == (want.acc_oob, want.loss_ib)


@pytest.mark.parametrize("key", list(T.PLUGIN_CASES))
def test_training_entries_every_width(key, oracle):
    """build_set_haplo_geno + build_acc_oob / build_acc_ib / build_haplomatch through the table, as above, on generated
    inputs: n_snp = 1, 2, 31...33, 63...65, 95...97, 127, 128 at 65 samples (two sample groups, one of them a single lane)
    and 1, 63, 64, 65, 130 samples at 65 SNPs.  Both packed words and both words of each genotype plane are filled, with
    the reference's garbage above n_snp in the haplotypes.  First under test because of these cases: build_eval<2>
    (33...64 SNPs), <3> (65...96), <4> (97...128) -- the [w * n_haplo + a] strides against the NW-strided planes, bits 0
    and 31 of every word, the mask of the top word -- and match_dist with nw > 1.  In "far" one out-of-bag sample is far
    from every pair: no best guess, which counts as no correct allele; its NaN posterior stays out of the in-bag sum."""
    _check_entries(key, T.plugin_case(key), T.case_score(key))


def test_haplomatch_beyond_the_pair_bound(oracle):
    """The same on "two-pass" (T.MATCH_CASES): 1,100 haplotypes, a pair bound of 4.6 million -- past 1 << 20, where
    build_haplomatch counts the pairs in an operation of its own, sums the counts on the host and writes the pairs in a
    second one.  That path uploads into the buffers build_set_haplo_geno fills, so the two scores are taken once more after
    it and must come out the same."""
    _check_entries("two-pass", T.match_case("two-pass"), T.match_score("two-pass"), scores_again=True)


def test_haplomatch_without_in_bag_samples(oracle):
    """build_set_bootstrap with all zeros: build_haplomatch returns the empty list (buf[0] == 0, out_n == 1), and the state
    is as usable afterwards as before -- the case's own counts and a build_set_haplo_geno give the case's scores."""
    cs, want = T.plugin_case("snp33"), T.case_score("snp33")
    with _Entries(cs) as e:
        e.bootstrap(np.zeros(len(cs.boot), np.int32))
        pairs, out_n = e.haplomatch()
        e.bootstrap(cs.boot)
        got = e.scores()
    print(f"no in-bag sample: buffer {pairs.tolist()}, out_n {out_n}; then acc_oob {got[0]}, acc_ib {got[1]!r}")
    assert pairs.tolist() == [0] and out_n == 1
    assert got == (want.acc_oob, want.loss_ib)
