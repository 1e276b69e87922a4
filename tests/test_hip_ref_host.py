"""The plugin table driven by the reference's own host code (GPU).

The ten ``TypeGPUExtProc`` entries (inst/include/LibHLA_ext.h:358-388) were only ever called by Python imitations of the
host (hibag_amd/plugin.py, the loops of tests/test_hip_training.py).  Here the HIBAG library itself --
``oracle/_ref/libhibag_ref.so``, compiled from the package sources by ``oracle.build_ref()`` where those are present --
gets ``GPUExtProcPtr = hibag_hip_gpu_ext_proc()`` and runs its ``PredictHLA`` and ``BuildClassifiers`` through the table.
What it computes with the table must equal, as bits, what the same library computes on the CPU with the pointer cleared
and the target ``base``.

Only the built library is used, never the package sources; without it the tests skip."""

import ctypes as C
import os

import numpy as np
import pytest

import ref_cases as RC

pytestmark = pytest.mark.gpu

# field order of TypeGPUExtProc
ENTRIES = ("build_init", "build_done", "build_set_bootstrap", "build_haplomatch", "build_set_haplo_geno",
           "build_acc_oob", "build_acc_ib", "predict_init", "predict_done", "predict_avg_prob")


@pytest.fixture(scope="module")
def ref(oracle):
    if not os.path.exists(oracle.REF_LIB_PATH):
        pytest.skip("oracle/_ref/libhibag_ref.so is not built (oracle.build_ref() needs the HIBAG package sources)")
    import hibag_amd
    from oracle import ref as R
    hibag_amd.hlaSetKernelTarget("hip")
    R.lib(oracle.REF_LIB_PATH)
    yield R
    R.reset()


@pytest.fixture
def host(ref, request):
    """The reference on its ``base`` target with no plugin; global target and plugin pointer are put back afterwards."""
    request.addfinalizer(ref.reset)
    ref.set_gpu_table(None)
    ref.set_target("base")
    return ref


def table(keep=ENTRIES):
    """A copy of the project's table with every entry outside ``keep`` set to NULL (the reference tests each entry on its
    own: src/LibHLA.cpp:1014, :1916, :1938, :1961, :2258-2293, :2433, :2500, :2527)."""
    from hibag_amd import _lib
    src = (C.c_void_p * len(ENTRIES)).from_address(_lib.lib().hibag_hip_gpu_ext_proc())
    t = (C.c_void_p * len(ENTRIES))()
    for i, name in enumerate(ENTRIES):
        assert src[i], name
        t[i] = src[i] if name in keep else None
    return t


def _predict_through_the_plugin(host, model, G, what):
    with host.Model.from_obj(model) as m:
        cpu = m.predict(G, 1)
        cpu2 = m.predict(G, 2)
        t = table()
        host.set_gpu_table(C.addressof(t))
        gpu1 = m.predict(G, 1)
        gpu2 = m.predict(G, 2)
        host.set_gpu_table(None)
        again = m.predict(G, 1)
    RC.assert_same_bits(again, cpu, f"{what}: the CPU route after the plugin was cleared")
    RC.assert_same_bits(gpu1, cpu, f"{what}: PredictHLA through predict_init / predict_avg_prob / predict_done")
    # the reference's GPU branch never looks at vote_method (src/LibHLA.cpp:2433-2441): vote 2 gives the vote-1 arrays
    RC.assert_same_bits(gpu2, gpu1, f"{what}: vote 2 through the plugin")
    assert not np.array_equal(cpu2["postprob"], cpu["postprob"], equal_nan=True)      # (which the CPU route tells apart)
    return cpu


def test_predict_through_the_reference_host(host):
    """Classifiers of 1, 31, 32, 33, 64, 65 and 128 SNPs and one with nothing in it, 24 samples (5 % missing, sample 3 all
    NA); then a model with a 150-haplotype classifier, whose 11,325 pairs take predict_avg_prob's kernel two rounds."""
    from hibag_amd.model import Classifier
    model, G = RC.width_model(24, [1, 31, 32, 33, 64, 65, 128], seed=81)
    model.classifiers.insert(4, Classifier(np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32), []))
    assert len(model.classifiers) == 8 and G.shape[0] == 24
    cpu = _predict_through_the_plugin(host, model, G, "widths")
    assert np.isnan(cpu["matching"][3]) and np.isfinite(np.delete(cpu["matching"], 3)).all()

    from hibag_amd import synth
    big, founders, af = synth.make_model("hla-a-small", seed=83, n_classifier=3, n_snp=60, n_haplo=150, wide_classifier=False)
    assert all(len(c.freq) == 150 for c in big.classifiers)
    Gb, _ = synth.make_samples(founders, af, 8, seed=84, miss=0.05)
    _predict_through_the_plugin(host, big, Gb, "150 haplotypes")


def _train(host, keep, record=False, counted=None):
    """BuildClassifiers on the cohort with the entries of ``keep`` (None: no plugin).  ``counted``: a dict that receives how
    often the host called build_acc_oob and build_acc_ib."""
    G, a1, a2, n_hla = RC.training_cohort()
    if keep is not None:
        t = table(keep)
        if counted is not None:
            wrappers = []
            for name, restype in (("build_acc_oob", C.c_int), ("build_acc_ib", C.c_double)):
                i = ENTRIES.index(name)
                real = C.CFUNCTYPE(restype)(t[i])
                counted[name] = 0

                def call(real=real, name=name):
                    counted[name] += 1
                    return real()
                wrappers.append(C.CFUNCTYPE(restype)(call))
                t[i] = C.cast(wrappers[-1], C.c_void_p).value
        host.set_gpu_table(C.addressof(t), record=record)
    try:
        with host.Model.for_training(G, a1, a2, n_hla) as m:
            out = m.train(3, 8, prune=True, seed=100)
        calls = host.match_calls() if record else None
    finally:
        host.set_gpu_table(None)
    return (out, calls) if record else out


def test_scoring_through_the_reference_search(host):
    """BuildClassifiers (80 samples x 60 SNPs, 3 classifiers, mtry 8) with every entry but build_haplomatch: the host makes
    its pair lists on the CPU and scores every candidate SNP with build_set_haplo_geno / build_acc_oob / build_acc_ib.  The
    model must be the CPU run's: SNPs in order, bootstrap counts, haplotype bits below k, frequencies, alleles, accuracies."""
    cpu = _train(host, None)
    counted = {}
    gpu = _train(host, [e for e in ENTRIES if e != "build_haplomatch"], counted=counted)
    RC.assert_same_training(gpu, cpu, "scoring entries")
    print(f"the host called {counted}")
    # the entries did the scoring: build_acc_oob for every candidate, build_acc_ib for those that do not lower the accuracy
    # (src/LibHLA.cpp:2030-2034) -- at least once for each SNP that was kept
    kept = sum(len(c["snpidx"]) for c in cpu)
    assert counted["build_acc_oob"] >= counted["build_acc_ib"] >= kept >= 3 * 4


def test_haplomatch_through_the_reference_search(host, oracle):
    """With build_haplomatch the host expands the plugin's pairs in another order than its CPU branch makes them
    (src/LibHLA.cpp:1044-1060 against :1104-1122) and the EM sums depend on the order, so the CPU run is no reference here.
    Instead: the full table's model equals, bit for bit, that of a table with build_init, build_done, build_set_bootstrap
    and build_haplomatch only (the reference scores on the CPU then); and every recorded build_haplomatch call, replayed
    through the oracle's _PrepHaploMatch, has the same pairs in the same order for each in-bag sample, none of them empty,
    and out_n == 1 + 2 * count."""
    full, calls = _train(host, ENTRIES, record=True)
    hybrid = _train(host, ["build_init", "build_done", "build_set_bootstrap", "build_haplomatch"])
    RC.assert_same_training(full, hybrid, "full table against the match-only table")

    assert len(calls) >= 3 * 2                       # at least two search steps per classifier
    n_pairs = 0
    for ci, call in enumerate(calls):
        k, lens, geno, buf = call["n_snp"], call["lens"], call["geno"], call["buf"]
        assert buf is not None, f"call {ci}: NULL buffer"
        cnt = int(buf[0]) // 2
        assert call["out_n"] == 1 + 2 * cnt and len(buf) == 1 + 2 * cnt, f"call {ci}"
        got = {}
        for s, v in buf[1:].reshape(-1, 2):
            got.setdefault(int(s), []).append((int(v) & 0xFFFF, int(v) >> 16))
        H = int(lens.sum())
        assert len(call["haplo"]) == H
        bits = np.ascontiguousarray(call["haplo"]["bits"] & host.low_mask(k))
        fm = oracle.FlatModel(len(lens), 1, k, np.array([k], np.int32), np.array([0, k], np.int32), np.arange(k, dtype=np.int32),
                              np.array([0, H], np.int32), lens.astype(np.int32)[None, :], bits,
                              np.ascontiguousarray(call["haplo"]["freq"]))
        st = np.concatenate([[0], np.cumsum(lens)])
        inbag = np.flatnonzero(geno["boot"] > 0)
        assert len(inbag) and set(got) == set(range(len(inbag))), f"call {ci}: a sample without pairs, or one too many"
        for kk, s in enumerate(inbag):
            a1, a2 = int(geno["a1"][s]), int(geno["a2"][s])
            assert a1 <= a2                            # the host orders each sample's alleles (src/LibHLA.cpp:1054)
            want = oracle.prep_haplo_match(fm, 0, geno["s1"][s], geno["s2"][s], a1, a2)
            want = [(int(i) - int(st[a1]), int(j) - int(st[a2])) for i, j in want]
            assert len(want) >= 1 and got[kk] == want, f"call {ci} ({k} SNPs), in-bag sample {kk}"
            n_pairs += len(want)
    print(f"{len(calls)} build_haplomatch calls replayed, {n_pairs} pairs")
