"""What tests/test_edge_corpus_host.py (CPU) and tests/test_hip_edge_corpus.py (GPU) share: the inputs that go with the cases of
``ref_cases.PREDICT_CASES`` in each derived entry -- bootstrap counts, classifier masks, the knock-out's cut of the model, the
second model of a merge, the list lengths, partitions, allele sets and pedigrees of the five entries with a finish of their
own -- and each entry's reference result, computed once per session from the oracle alone and handed out read-only."""

import dataclasses

import numpy as np

import curve_reference as CR
import draws_reference as DR
import family_reference as FR
import given_reference as GR
import groups_reference as GPR
import importance_reference as IR
import masked_reference as MR
import predmerge_reference as PR
import ref_cases as RC
import topk_reference as TR
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


# ---- the finishes with kernels of their own: top-k, draws, groups, given, family ------------------------------------------
# Each reads the oracle's posterior matrix of the case and applies the entry's numpy restatement to it.
LANE_CASES = ["subnormal-lanes", "mixed-lanes", "mixed-lanes-each"]
HEALTHY, INF, NAN, MISSING, OUT = 0, 1, 2, 3, -1
KIND_NAMES = {HEALTHY: "healthy", INF: "inf", NAN: "nan", MISSING: "missing", OUT: "not in the call"}


def n_hla(name):
    return int(case(name)[0].n_hla)


def posterior(name, vote):
    """(posterior matrix [n_samp, n_cell], matching [n_samp]) of the oracle."""
    r = plain_want(name, vote)
    return r["postprob"], r["matching"]


def draw_S(name, vote):
    """The draw reference's S: the sequential sum of a sample's posterior in cell order."""
    return _once(("S", name, vote), lambda: np.cumsum(posterior(name, vote)[0], axis=1)[:, -1])


def row_kinds(name):
    """int [n_samp]: what a sample's row of the vote-1 posterior is -- INF (a +inf cell; the empty cells beside it are NaN
    in the mixed cases), NAN (NaN cells and no inf: a total of 0), MISSING (no positive cell: nothing typed) or HEALTHY."""
    def make():
        pp, _ = posterior(name, 1)
        inf = np.isposinf(pp).any(axis=1)
        nan = np.isnan(pp).any(axis=1) & ~inf
        with np.errstate(invalid="ignore"):
            missing = ~inf & ~nan & ~(pp > 0).any(axis=1)
        return np.where(inf, INF, np.where(nan, NAN, np.where(missing, MISSING, HEALTHY)))
    return _once(("kinds", name), make)


# -- top-k: a k for each compiled list length of k_finish_topk (4, 8, 16), 16 being above the small cases' six cells
TOPK_K = [1, 4, 5, 16]


def topk_want(name, vote, k):
    def make():
        pp, mt = posterior(name, vote)
        return {**TR.select(pp, k, n_hla(name)), "matching": mt}
    return _once(("topk", name, vote, k), make)


# -- draws: an n for each workgroup shape of k_finish_draw (one, two, four wavefronts of 16 draws); a seed with a high word;
# sample 0 of the caller's numbering, and one from which the counter's low word runs over into its high word at lane 64
DRAW_N = [1, 16, 17, 64]
DRAW_SEED = 0x9E3779B97F4A7C15
DRAW_SAMPLE0 = [0, (3 << 32) + 0xFFFFFFC0]


def draws_all(name, vote, sample0):
    """``draws_reference.draws_from_postprob`` with n = 64: draw t is a function of (seed, sample, t) and the posterior alone,
    so its first n columns are the call with n draws (tests/test_edge_corpus_host.py holds it to that)."""
    def make():
        pp, mt = posterior(name, vote)
        return {**DR.draws_from_postprob(pp, max(DRAW_N), DRAW_SEED, sample0, n_hla(name)), "matching": mt}
    return _once(("draws", name, vote, sample0), make)


def draws_want(name, vote, n, sample0):
    def make():
        full = draws_all(name, vote, sample0)
        return {k: (v if v.ndim == 1 else np.ascontiguousarray(v[:, :n])) for k, v in full.items()}
    return _once(("draws-n", name, vote, sample0, n), make)


# -- groups: one plan of five partitions
IDENTITY, COARSE, SINGLE, WITH_EMPTY, RANDOM = range(5)


def partitions(name):
    """int32 [5, n_hla]: the identity, groups of three alleles, one group, groups 0 and 2 with group 1 empty, seeded ids."""
    n = n_hla(name)
    h = np.arange(n)
    rnd = np.random.default_rng(23).integers(0, max(2, n // 4), n)
    return np.stack([h, h // 3, np.zeros(n, np.int64), 2 * (h % 2), rnd]).astype(np.int32)


def groups_offsets(name):
    return np.concatenate([[0], np.cumsum(GPR.levels_of(partitions(name)))])


def groups_want(name, vote):
    def make():
        pp, mt = posterior(name, vote)
        return {**GPR.groups_from_postprob(pp, n_hla(name), partitions(name), True), "matching": mt}
    return _once(("groups", name, vote), make)


# -- given: five set pairs per sample
GIVEN_SETS = ["full", "random", "moved", "nan-only", "empty"]


def given_sets(name, which):
    """bool [n_samp, 2, n_hla].  "full": both sets every allele.  "random": a seeded coin per allele.  "moved": a sample
    with an inf cell, called (c1, c2), gets A = every allele but c1 and c2 and B full, which leaves every cell consistent but
    (c1, c1), (c1, c2) and (c2, c2), so the call has to move on; the others a seeded coin.  "nan-only": a sample with inf and
    NaN cells gets A = {a}, B = {b} of its first NaN cell (a, b), so its one consistent cell is NaN; the others a seeded
    coin.  "empty": A empty, B empty, both empty, in turn."""
    def make():
        n, nh = len(case(name)[1]), n_hla(name)
        pp, _ = posterior(name, 1)
        call = plain_want(name, 1)
        sets = np.ones((n, 2, nh), np.bool_)
        if which == "random":
            sets = np.random.default_rng(41).random((n, 2, nh)) < 0.6
        elif which == "moved":
            sets = np.random.default_rng(42).random((n, 2, nh)) < 0.7
            for s in np.nonzero(np.isposinf(pp).any(axis=1))[0]:
                sets[s] = True
                sets[s, 0, [call["h1"][s], call["h2"][s]]] = False
        elif which == "nan-only":
            sets = np.random.default_rng(43).random((n, 2, nh)) < 0.5
            h1, h2 = GR.cell_pairs(nh)
            for s in np.nonzero(np.isposinf(pp).any(axis=1) & np.isnan(pp).any(axis=1))[0]:
                c = int(np.isnan(pp[s]).argmax())
                sets[s] = False
                sets[s, 0, h1[c]] = sets[s, 1, h2[c]] = True
        elif which == "empty":
            sets[0::3, 0] = False
            sets[1::3, 1] = False
            sets[2::3] = False
        else:
            assert which == "full", which
        return sets
    return _once(("given-sets", name, which), make)


def given_want(name, vote, which):
    def make():
        pp, mt = posterior(name, vote)
        return {**GR.given_from_postprob(pp, n_hla(name), given_sets(name, which), True), "matching": mt}
    return _once(("given", name, vote, which), make)


# -- family
def family_case(name):
    """(rows [m], pedigree int32 [m, 2]): the call's sample i is the case's sample rows[i].

    The lane cases: the case's own samples in place, as founders; behind them, for every ordered pair of parent kinds the case
    has (OUT, HEALTHY, INF, NAN, MISSING) and every kind of child, a copy of a sample of the child's kind whose parents are
    samples of the pair's kinds (a kind's samples are taken from the last one down, so the first parents stand in the
    children's own 64-sample group and later ones in others; the children of (OUT, OUT) are founders and join their kind);
    behind those, a grandchild of every child that has a parent in the call, with the row before that child as its other
    parent.  Every other case: every third sample is the child of the two before it."""
    def make():
        n = len(case(name)[1])
        if name not in LANE_CASES:
            ped = FR.founders_only(n)
            kids = np.arange(2, n, 3)
            ped[kids, 0], ped[kids, 1] = kids - 2, kids - 1
            return np.arange(n), ped
        kind = row_kinds(name)
        have = [k for k in (HEALTHY, INF, NAN, MISSING) if (kind == k).any()]
        own = {k: [int(s) for s in np.nonzero(kind == k)[0]] for k in have}          # the case's samples of a kind
        pool = {k: list(own[k]) for k in have}                                         # ... and the founders copied from them
        turn = {k: 0 for k in have}
        child_turn = {k: 0 for k in have}

        def parent(k, avoid=-1):
            while k != OUT:
                p = pool[k][-1 - turn[k] % len(pool[k])]
                turn[k] += 1
                if p != avoid:
                    return p
            return -1

        def child(k):
            child_turn[k] += 1
            return own[k][(child_turn[k] - 1) % len(own[k])]

        rows, ped = list(range(n)), [(-1, -1)] * n
        for ka in [OUT] + have:
            for kb in [OUT] + have:
                for kc in have:
                    f = parent(ka)
                    rows.append(child(kc))
                    ped.append((f, parent(kb, avoid=f)))
                    if ka == OUT and kb == OUT:
                        pool[kc].append(len(rows) - 1)
        m = len(rows)
        for j in range(n + 1, m):
            if max(ped[j]) >= 0:
                rows.append(child(have[j % len(have)]))
                ped.append((j, j - 1) if j % 2 else (j - 1, j))
        return np.array(rows, np.int64), np.array(ped, np.int32)
    return _once(("family-case", name), make)


def family_geno(name):
    return _once(("family-geno", name), lambda: np.ascontiguousarray(case(name)[1][family_case(name)[0]]))


def family_prior(name, with_prior):
    return FR.model_prior(case(name)[0]) if with_prior else None


def family_want(name, vote, with_prior):
    def make():
        pp, mt = posterior(name, vote)
        rows, ped = family_case(name)
        return {**FR.family_from_postprob(pp[rows], n_hla(name), ped, family_prior(name, with_prior)), "matching": mt[rows]}
    return _once(("family", name, vote, with_prior), make)
