"""The yardstick of the per-sample classifier mask (tests/masked_reference.py) pinned on the host: its corner columns
equal the oracle's own predictions, and the bundled reference models with their stored bootstrap counts are inputs on
which an ignored mask cannot pass."""
import numpy as np
import pytest

import masked_reference as MR
from conftest import align_geno
from hibag_amd import NA_INTEGER
from test_oob_host import oracle_oob


def _samp_num(model):
    return np.stack([np.asarray(c.samp_num, np.int32) for c in model.classifiers])


@pytest.mark.parametrize("vote", [1, 2])
def test_all_ones_column_is_the_full_model(oracle, model_oob, hapmap_geno, vote):
    G = align_geno(model_oob, hapmap_geno)
    use = np.ones((len(model_oob.classifiers), len(G)), np.uint8)
    want = oracle.predict(oracle.flatten(model_oob), G, vote, want_dosage=True, want_prob=True)
    assert MR.same_bits(MR.masked(model_oob, G, use, vote), want)
    assert MR.same_bits(MR.masked(model_oob, G, use, vote, avx2=False), want)


def test_single_classifier_column_is_the_one_classifier_model(oracle, model_oob, hapmap_geno):
    """Column s keeps one of the sample's out-of-bag classifiers alone: the yardstick equals hlaOutOfBag's
    per-classifier loop on the oracle (tests/test_oob_host.py oracle_oob) at that (classifier, sample)."""
    G = align_geno(model_oob, hapmap_geno)
    sn = _samp_num(model_oob)
    C, n = sn.shape
    want = oracle_oob(oracle, model_oob, G)
    checked = 0
    for shift in range(3):                                 # three different (classifier, sample) pairings
        use = np.zeros((C, n), np.uint8)
        pick = np.full(n, -1)
        for s in range(n):
            oob = np.flatnonzero(sn[:, s] == 0)
            pick[s] = oob[(s + shift) % len(oob)]
            use[pick[s], s] = 1
        got = MR.masked(model_oob, G, use, 1)
        rows = np.arange(n)
        assert np.array_equal(got["h1"], want["h1"][pick, rows])
        assert np.array_equal(got["h2"], want["h2"][pick, rows])
        assert MR.same_bits({"prob": got["prob"]}, {"prob": want["prob"][pick, rows]}, keys=("prob",))
        checked += n
    assert checked == 3 * n


def test_all_zero_column_is_the_all_missing_sample(oracle, model_a, hapmap_geno):
    G = align_geno(model_a, hapmap_geno)[:5]
    use = np.ones((len(model_a.classifiers), 5), np.uint8)
    use[:, 2] = 0
    got = MR.masked(model_a, G, use, 1)
    assert got["h1"][2] == NA_INTEGER and got["h2"][2] == NA_INTEGER and got["prob"][2] == 0 and np.isnan(got["matching"][2])
    miss = oracle.predict(oracle.flatten(model_a), np.full((1, G.shape[1]), NA_INTEGER, np.int32), 1)
    assert MR.same_bits({k: got[k][2:3] for k in MR.KEYS}, miss)


@pytest.mark.parametrize("which", ["oob", "modellist_a"])
def test_the_bundled_models_tell_an_ignored_mask_apart(which, oracle, model_oob, model_a, hapmap_geno):
    """Conditions on the inputs of tests/test_hip_masked.py: every training sample has an out-of-bag classifier, the
    mask columns are all different, and at least one out-of-bag call differs from the full (in-bag) model's."""
    model = model_oob if which == "oob" else model_a
    G = align_geno(model, hapmap_geno)
    use = _samp_num(model) == 0
    n_oob = use.sum(axis=0)
    assert n_oob.min() >= 1
    assert len({use[:, s].tobytes() for s in range(use.shape[1])}) == use.shape[1]
    got = MR.masked(model, G, use, 1)
    full = oracle.predict(oracle.flatten(model), G, 1, want_dosage=False, want_prob=False)
    differ = int(np.count_nonzero((got["h1"] != full["h1"]) | (got["h2"] != full["h2"])))
    print(which, "samples", len(G), "out-of-bag classifiers", int(n_oob.min()), "-", int(n_oob.max()), "calls differing", differ)
    assert differ >= 1
