"""The oracle pinned to the reference by execution (CPU).

oracle/*.c restates the reference's prediction and training; until now it was held to it by reading, by printed values and
by the models the package stores.  Here the HIBAG library sources themselves -- compiled as they are against stand-in R
headers by ``oracle.build_ref()`` into the ignored ``oracle/_ref/libhibag_ref.so`` -- run the same inputs through their
public classes (oracle/ref_driver.cpp), and every output must equal the oracle's as bits:

* ``PredictHLA`` against ``oracle.predict``, scalar and AVX2 ports, votes 1 and 2, under each of the reference's targets
  base, sse2, sse4, avx and avx2 (the AVX-512 targets fuse multiply and add and differ in the last bit: not compared);
* ``BuildClassifiers`` against ``oracle.train``, prune on and off, under base and avx2, both fed R's ``set.seed(100)``
  stream as the oracle restates it.

Where the package sources are present the library must be there (it is built on the spot: a failing build fails the
tests); without sources and without a library the tests skip."""

import math

import numpy as np
import pytest

import ref_cases as RC
from conftest import align_geno
from test_oracle_train import training_inputs


@pytest.fixture(scope="module")
def ref(oracle):
    path = oracle.build_ref()
    if path is None:
        pytest.skip(f"no HIBAG sources under {oracle.ref_dir()} and no oracle/_ref/libhibag_ref.so built earlier")
    from oracle import ref as R
    R.lib(path)
    yield R
    R.reset()


@pytest.fixture
def target(ref, request):
    """The reference's kernel target for one test; the library's global state is put back afterwards."""
    request.addfinalizer(ref.reset)
    info = ref.set_target(request.param)
    assert not ref.gpu_table_is_set()
    return request.param, info


TARGETS = pytest.mark.parametrize("target", ["base", "sse2", "sse4", "avx", "avx2"], indirect=True)


def _predict_both_ports(oracle, ref, model, G, what):
    fm = oracle.flatten(model)
    wants = {}
    with ref.Model.from_obj(model) as m:
        for vote in (1, 2):
            want = wants[vote] = m.predict(G, vote)
            RC.assert_same_bits(oracle.predict(fm, G, vote_method=vote), want, f"{what}, vote {vote}, scalar port")
            RC.assert_same_bits(oracle.predict(fm, G, vote_method=vote, avx2=True, n_threads=3), want,
                                f"{what}, vote {vote}, AVX2 port")
    return wants


@TARGETS
@pytest.mark.parametrize("case", list(RC.PREDICT_CASES))
def test_predict_equals_the_reference(case, target, oracle, ref):
    model, G = RC.PREDICT_CASES[case]()
    want = _predict_both_ports(oracle, ref, model, G, f"{case} under {target[0]}")
    if case == "underflow":
        assert np.isnan(want[1]["postprob"][0]).all() and want[1]["h1"][0] == oracle.NA_INTEGER
    if case == "widths":
        assert sorted(len(c.snpidx) for c in model.classifiers) == RC.WIDTHS and len(G) == 60


@TARGETS
def test_predict_bundled_model_equals_the_reference(target, oracle, ref, hapmap_geno, model_a):
    """The bundled HLA-A model (inst/extdata/ModelList.RData) on the 60 HapMap CEU samples."""
    G = align_geno(model_a, hapmap_geno, hapmap_geno.sample_id)
    _predict_both_ports(oracle, ref, model_a, G, f"bundled HLA-A under {target[0]}")


def test_target_names_reach_the_named_kernels(ref):
    """The five targets are five code paths, not one: the library describes what it selected."""
    seen = {t: ref.set_target(t) for t in ref.TARGETS}
    ref.reset()
    assert "SSE" not in seen["base"] and "AVX" not in seen["base"]
    assert seen["sse2"].endswith("SSE2") or "SSE2," in seen["sse2"]
    assert "SSE4.2" in seen["sse4"] and "AVX2" in seen["avx2"]
    assert "AVX" in seen["avx"] and "AVX2" not in seen["avx"]


TRAIN_TARGETS = pytest.mark.parametrize("target", ["base", "avx2"], indirect=True)


@TRAIN_TARGETS
@pytest.mark.parametrize("prune", [True, False])
def test_training_equals_the_reference_on_a_synthetic_cohort(prune, target, oracle, ref):
    G, a1, a2, n_hla = RC.training_cohort()
    assert G.shape == (80, 60)
    with ref.Model.for_training(G, a1, a2, n_hla) as m:
        want = m.train(3, 8, prune=prune, seed=100)
    got = oracle.train(G, a1, a2, n_hla, nclassifier=3, mtry=8, prune=prune, seed=100)
    RC.assert_same_training(got, want, f"prune {prune} under {target[0]}")
    assert max(len(c["snpidx"]) for c in want) >= 4 and max(len(c["freq"]) for c in want) > n_hla       # a real search


@TRAIN_TARGETS
@pytest.mark.parametrize("prune", [True, False])
def test_training_equals_the_reference_on_the_vignette_call(prune, target, oracle, ref, hapmap_geno, hla_type_table, model_oob):
    """set.seed(100); hlaAttrBagging(hlatab$training, train.geno, ...) on the fixture data (vignettes/HIBAG.Rmd:218-220),
    the first classifiers: with prune on these are also the ones the package stores (tests/test_oracle_train.py)."""
    G, a1, a2 = training_inputs(model_oob, hapmap_geno, hla_type_table)
    mtry = math.ceil(math.sqrt(model_oob.n_snp))
    n = 8
    with ref.Model.for_training(G, a1, a2, model_oob.n_hla) as m:
        want = m.train(n, mtry, prune=prune, seed=100)
    got = oracle.train(G, a1, a2, model_oob.n_hla, nclassifier=n, mtry=mtry, prune=prune, seed=100)
    RC.assert_same_training(got, want, f"vignette, prune {prune} under {target[0]}")
    if prune:
        for i, (w, stored) in enumerate(zip(want, model_oob.classifiers)):
            assert np.array_equal(w["snpidx"], stored.snpidx) and np.array_equal(w["freq"], stored.freq), i
            assert w["acc"] == stored.outofbag_acc, i


def test_a_throwing_run_reports_and_clears_the_plugin_pointer(ref):
    """The driver's exception path: the reference throws ErrHLA for a bad vote method; the message is kept, and a plugin
    table that was set is not left installed."""
    import ctypes as C
    model, G = RC.underflow_model()
    empty = (C.c_void_p * 10)()                     # a table with no entry: the CPU branches everywhere
    try:
        ref.set_gpu_table(C.addressof(empty))
        assert ref.gpu_table_is_set()
        with ref.Model.from_obj(model) as m:
            with pytest.raises(ref.RefError, match="Invalid 'vote_method'."):
                m.predict(G, 3)
        assert not ref.gpu_table_is_set()
    finally:
        ref.reset()
