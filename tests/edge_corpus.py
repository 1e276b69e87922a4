"""What tests/test_edge_corpus_host.py (CPU) and tests/test_hip_edge_corpus.py (GPU) share: the inputs that go with the cases of
``ref_cases.PREDICT_CASES`` in each derived entry -- bootstrap counts, classifier masks, the knock-out's cut of the model, the
second model of a merge -- and each entry's reference result, computed once per session from the oracle alone and handed
out read-only."""

import dataclasses

import numpy as np

import curve_reference as CR
import importance_reference as IR
import masked_reference as MR
import predmerge_reference as PR
import ref_cases as RC
from hibag_amd import synth
from hibag_amd.merge import merge_plan
from oracle import oracle as O
from test_oob_host import oracle_oob

CASES = list(RC.PREDICT_CASES)
NEW_CASES = ["subnormal", "subnormal-lanes", "mixed-lanes", "mixed-lanes-each"]
KNOCK_CUT = [0, 3, 6, 1]               # mixed-lanes in the knock-out: one-step matrix engine, several K steps, int8, VALU

_cache = {}


def _once(key, make, freeze=True):
    if key not in _cache:
        _cache[key] = _frozen(make()) if freeze else make()
    return _cache[key]


def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _frozen(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _frozen(v)
    return x


def case(name):
    """(model, G) of a corpus case."""
    return _once(("case", name), RC.PREDICT_CASES[name])


# ---- the curve ------------------------------------------------------------------------------------------------------------
def curve_want(name):
    return _once(("curve", name), lambda: CR.curve(*case(name)))


# ---- out of bag -----------------------------------------------------------------------------------------------------------
def samp_num(name, boot):
    """Bootstrap counts [C, n]: ``boot`` "seeded" (``masked_reference.bootstrap``) or "all-out" (everybody out of bag)."""
    model, G = case(name)
    C, n = len(model.classifiers), len(G)
    return MR.bootstrap(C, n, seed=100 + n) if boot == "seeded" else np.zeros((C, n), np.int32)


def with_samp_num(model, sn):
    return dataclasses.replace(model, classifiers=[dataclasses.replace(c, samp_num=np.asarray(r, np.int32))
                                                   for c, r in zip(model.classifiers, sn)])


def oob_want(name, boot):
    def make():
        model, G = case(name)
        return oracle_oob(O, with_samp_num(model, samp_num(name, boot)), G, avx2=True, n_threads=8)
    return _once(("oob", name, boot), make)


# ---- the knock-out --------------------------------------------------------------------------------------------------------
def knock_case(name):
    """(model with bootstrap counts, G, truth): mixed-lanes cut to the classifiers ``KNOCK_CUT``, renumbered; the truth is
    every sample's call by that model where there is one (the tallies need a truth, not a right one)."""
    def make():
        model, G = case(name)
        keep = KNOCK_CUT if name.startswith("mixed-lanes") else range(len(model.classifiers))
        model = dataclasses.replace(model, classifiers=[model.classifiers[c] for c in keep])
        sn = MR.bootstrap(len(model.classifiers), len(G), seed=300 + len(G))
        sn[:, ::2] = 0                                   # every other sample is out of every bag
        model = with_samp_num(model, sn)
        r = O.predict(O.flatten(model), np.ascontiguousarray(G), 1, want_dosage=False, want_prob=False)
        truth = np.stack([r["h1"], r["h2"]], axis=1).astype(np.int32)
        return model, G, truth
    return _once(("knock-case", name), make)


def knock_want(name):
    def make():
        model, G, _ = knock_case(name)
        return IR.knock_raw(O, model, G, avx2=True, n_threads=8)
    return _once(("knock", name), make)


# ---- the mask -------------------------------------------------------------------------------------------------------------
def mask(name):
    """uint8 [C, n]: a seeded coin per (classifier, sample); sample 0 keeps every classifier and the last sample none."""
    model, G = case(name)
    use = np.random.default_rng(17).integers(0, 2, (len(model.classifiers), len(G))).astype(np.uint8)
    use[:, 0] = 1
    use[:, -1] = 0
    return use


def masked_want(name, vote):
    return _once(("masked", name, vote), lambda: MR.masked(*case(name), mask(name), vote))


def plain_want(name, vote):
    return _once(("plain", name, vote), lambda: O.predict(O.flatten(case(name)[0]), np.ascontiguousarray(case(name)[1]), vote,
                                                          want_dosage=True, want_prob=True))


# ---- the merge ------------------------------------------------------------------------------------------------------------
MERGE_WEIGHT = [0.7, 1.9]


def merge_models(name):
    """(the case's model, an ordinary second model on the same SNPs): the second has nine alleles of which five carry names
    of the first's (every other one), so some merged rows have two sources, some one and the cross-model pairs none."""
    def make():
        model, _ = case(name)
        model = dataclasses.replace(model, hla_locus="A")
        other, _, _ = synth.make_model("hla-a-small", seed=31, n_hla=9, n_snp=model.n_snp, n_classifier=6, wide_classifier=False)
        shared = list(model.hla_allele[::2][:5])
        other.hla_allele = shared + [f"77:{i + 1:02d}" for i in range(9 - len(shared))]
        other.hla_locus = "A"
        return model, other
    return _once(("merge-models", name), make, freeze=False)


def merge_inputs(name):
    """(plan, posteriors [n_cell_i, n] and matchings [n] of both models) from the oracle."""
    def make():
        models = merge_models(name)
        G = np.ascontiguousarray(case(name)[1])
        plan = merge_plan([m.hla_allele for m in models])
        res = [O.predict(O.flatten(m), G, 1, want_dosage=False, want_prob=True) for m in models]
        return plan, [np.ascontiguousarray(r["postprob"].T) for r in res], [r["matching"] for r in res]
    return _once(("merge-inputs", name), make)


def merge_want(name, use_matching):
    def make():
        plan, pp, mt = merge_inputs(name)
        return PR.merge_reference(pp, mt, MERGE_WEIGHT, plan.row_of_cell, len(plan.hla_allele), use_matching=use_matching)
    return _once(("merge", name, use_matching), make)
