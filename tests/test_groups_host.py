"""hlaPredictGroups without a GPU: the reference of the group calls (tests/groups_reference.py) reduces to the oracle's own
call, probability and dosage on the identity partition; the corner the GPU tests stand on is there (a collapsed call differs
from the relabelled allele call); the constructors of HlaAlleleGroups."""
import numpy as np
import pytest

from conftest import align_geno
from groups_reference import NA_INTEGER, groups, groups_from_postprob, relabelled
from hibag_amd import synth
from hibag_amd.groups import HlaAlleleGroups, hlaGroupsByMap, hlaGroupsByResolution, hlaGroupsBySequence
from hibag_amd.merge import hlaAlleleDigit
from hibag_amd.model import Classifier, HlaAttrBagObj

NA = NA_INTEGER


def underflow_case():
    """A classifier whose every pair is >= 65 mismatches away has total 0: 1/total = inf and 0 * inf = NaN poisons the whole
    sample (the recipe of tests/test_hip_draws.py)."""
    k = 100
    far = Classifier(np.arange(k), [0.5, 0.5], [0, 1], ["1" * k, "1" * k])
    near = Classifier(np.arange(4), [0.3, 0.3, 0.4], [0, 1, 2], ["0000", "0101", "1111"])
    model = HlaAttrBagObj(0, k, ["a", "b", "c"], [near, far])
    G = np.zeros((3, k), np.int32)
    G[1, 40:] = NA
    G[2, :] = NA
    return model, G


def assert_identity(model, G, vote, what):
    r = groups(model, G, np.arange(model.n_hla, dtype=np.int32)[None, :], vote=vote)
    call = r["call"]
    for key, mine in (("h1", r["g1"][:, 0]), ("h2", r["g2"][:, 0]), ("prob", r["prob"][:, 0]), ("dosage", r["dosage"])):
        assert np.array_equal(mine, call[key], equal_nan=True), (what, vote, key)
    return r


@pytest.mark.parametrize("which", ["model_a", "model_oob"])
def test_identity_partition_is_the_oracles_own_call_and_dosage(which, request, hapmap_geno, oracle):
    model = request.getfixturevalue(which)
    G = align_geno(model, hapmap_geno, hapmap_geno.sample_id)
    for vote in (1, 2):
        assert_identity(model, G, vote, which)


def test_identity_partition_on_nan_posteriors(oracle):
    model, G = underflow_case()
    r = assert_identity(model, G, 1, "underflow")
    assert np.isnan(r["postprob"][0]).all() and r["g1"][0, 0] == NA and r["prob"][0, 0] == 0.0     # the corner is there
    assert np.isnan(r["dosage"][0]).all()
    assert r["g1"][2, 0] == NA and r["prob"][2, 0] == 0.0 and np.all(r["dosage"][2] == 0.0)         # all missing


def test_the_corner_is_there(oracle):
    """Posteriors spread over many alleles: the collapsed call is another one than the relabelled allele call in many
    samples, and never less probable.  Without this every GPU test would pass on a relabelling."""
    model, founders, af = synth.make_model("hla-a-small", seed=11)
    G, _ = synth.make_samples(founders, af, 130, seed=12, miss=0.85)
    G[77, :] = NA
    h = np.arange(model.n_hla)
    parts = np.stack([h % 3, h // 2, h % 2]).astype(np.int32)
    r = groups(model, G, parts, vote=1, want_dosage=False)
    call = r["call"]
    ok = call["h1"] != NA
    assert ok.sum() == 129 and not ok[77]
    counts = []
    for q in range(3):
        a, b = relabelled(call["h1"], call["h2"], parts[q])
        differ = ok & ((a != r["g1"][:, q]) | (b != r["g2"][:, q]))
        counts.append(int(differ.sum()))
        assert np.all(r["prob"][ok, q] >= call["prob"][ok]), q
        assert np.all(r["g1"][~ok, q] == NA) and np.all(r["prob"][~ok, q] == 0.0), q
    print("samples whose collapsed call differs from the relabelled call (h % 3, h // 2, h % 2):", counts,
          "median probability", float(np.median(call["prob"][ok])), "->", float(np.median(r["prob"][ok, 0])))
    assert counts[0] >= 10 and counts[1] >= 10, counts


# ---- constructors ---------------------------------------------------------------------------------------------------
ALLELES = ["01:01", "02:01", "01:02", "03:01:01", "02:05N", "24:02"]


def test_groups_by_resolution_is_hla_allele_digit():
    g = hlaGroupsByResolution(ALLELES, "2-digit")
    digits = hlaAlleleDigit(ALLELES, "2-digit")
    assert g.names == ["2-digit"] and g.n_part == 1 and g.alleles == ALLELES
    assert g.levels == [["01", "02", "03", "24"]]                    # first appearance along the alleles, not sorted
    assert g.group_of.dtype == np.int32 and g.group_of.tolist() == [[0, 1, 0, 2, 1, 3]]
    assert g.labels(0) == digits
    four = hlaGroupsByResolution(ALLELES, "4-digit", rm_suffix=True)
    assert four.labels("4-digit") == hlaAlleleDigit(ALLELES, "4-digit", rm_suffix=True) and "02:05" in four.levels[0]
    with pytest.raises(ValueError):
        hlaGroupsByResolution(ALLELES, "5-digit")

    class Model:
        hla_allele = ALLELES
    assert hlaGroupsByResolution(Model(), "2-digit").group_of.tolist() == g.group_of.tolist()


def test_groups_by_map_keeps_unmapped_names():
    g = hlaGroupsByMap(ALLELES, {"01:01": "Bw4", "24:02": "Bw4", "02:01": "Bw6"}, "Bw")
    assert g.names == ["Bw"] and g.levels == [["Bw4", "Bw6", "01:02", "03:01:01", "02:05N"]]
    assert g.group_of.tolist() == [[0, 1, 2, 3, 4, 0]]


def test_groups_by_sequence():
    seq = {"01:01": "MAVLTSRW", "02:01": "MAVMTSRW", "01:02": "MAVLTSGW", "03:01:01": "MGVLTSRW", "24:02": "MAVLTSRW",
           "99:99": "XXXXXXXX"}                                      # 02:05N has no sequence; 99:99 is not in the model
    g = hlaGroupsBySequence(ALLELES, seq, first=-2)                  # position of character i: -2 + i
    assert g.names == ["-1", "1", "4"]                               # characters 1, 3 and 6; the monomorphic ones are skipped
    assert g.levels == [["A", "G", "?"], ["L", "M", "?"], ["R", "G", "?"]]
    assert g.group_of.tolist() == [[0, 0, 0, 1, 2, 0], [0, 1, 0, 0, 2, 0], [0, 0, 1, 0, 2, 0]]
    assert g.n_level == 9 and g.offsets.tolist() == [0, 3, 6, 9]
    one = hlaGroupsBySequence(ALLELES, seq, positions=[4, -2], first=-2)
    assert one.names == ["4", "-2"] and one.levels[1] == ["M", "?"] and one.group_of[0].tolist() == g.group_of[2].tolist()
    with pytest.raises(ValueError):
        hlaGroupsBySequence(ALLELES, seq, positions=[6], first=-2)
    with pytest.raises(ValueError):
        hlaGroupsBySequence(ALLELES, dict(seq, **{"01:01": "MAV"}))
    with pytest.raises(ValueError):
        hlaGroupsBySequence(ALLELES, {a: "MMMM" for a in ALLELES})   # nothing polymorphic


def test_add_concatenates_and_a_matrix_is_taken_as_it_is():
    a, b = hlaGroupsByResolution(ALLELES, "2-digit"), hlaGroupsByMap(ALLELES, {"01:01": "x"}, "m")
    s = a + b
    assert s.names == ["2-digit", "m"] and s.levels == a.levels + b.levels and s.n_part == 2 and len(s) == 2
    assert np.array_equal(s.group_of, np.concatenate([a.group_of, b.group_of])) and s.index("m") == 1
    assert s.offsets.tolist() == [0, 4, 10]
    with pytest.raises(ValueError):
        a + hlaGroupsByResolution(ALLELES[:-1], "2-digit")
    raw = HlaAlleleGroups.from_matrix(ALLELES, [[5, 0, 0, 2, 2, 2], [0, 0, 0, 0, 0, 0]])
    assert raw.group_of.tolist() == [[5, 0, 0, 2, 2, 2], [0, 0, 0, 0, 0, 0]]          # not renumbered: ids 1, 3, 4 are empty groups
    assert raw.levels == [["0", "1", "2", "3", "4", "5"], ["0"]] and raw.names == ["partition1", "partition2"]
    assert HlaAlleleGroups.from_matrix(ALLELES, np.arange(6)).n_part == 1


@pytest.mark.parametrize("bad", [np.zeros((2, 5), np.int32), np.zeros((2, 6)), np.zeros((0, 6), np.int32),
                                 np.full((1, 6), 6, np.int32), np.full((1, 6), -1, np.int32), np.zeros((1, 2, 6), np.int32)])
def test_bad_shapes_and_ids_are_rejected(bad):
    with pytest.raises(ValueError):
        HlaAlleleGroups.from_matrix(ALLELES, bad)
    with pytest.raises(ValueError):
        HlaAlleleGroups(ALLELES, ["p"] * len(bad), [["x"] * 6] * len(bad), bad)


def test_reference_one_group_is_the_running_sum():
    rng = np.random.default_rng(5)
    pp = rng.random((7, 15))
    r = groups_from_postprob(pp, 5, np.zeros((1, 5), np.int32))
    assert np.array_equal(r["prob"][:, 0], np.cumsum(pp, axis=1)[:, -1]) and np.all(r["g1"] == 0) and np.all(r["g2"] == 0)
    assert r["dosage"].shape == (7, 1)
