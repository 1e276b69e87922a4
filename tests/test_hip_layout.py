"""The layout the host tests replay (tests/test_layout_host.py) is the layout the device gets: a model is planned, then the
SAME handle is finalized; the plan's scalars must be the finalized handle's, and the device's posterior on 70 samples must be the
posterior replayed from the plan's lists in float64, bit for bit -- under every HIBAG_PASS2 setting."""

import numpy as np
import pytest

import layout_reference as R
from test_layout_host import cohort, model_of, same_posterior, set_env

pytestmark = pytest.mark.gpu

ENGINE_NAME = {0: "valu", 1: "fp4", 2: "i8", 3: "i8"}


@pytest.mark.parametrize("pass2", [None, "stream", "hybrid", "recompute"])
@pytest.mark.parametrize("name", ["a_small", "widths", "only_wide", "empty"])
def test_the_exported_plan_is_what_the_device_runs(name, pass2, monkeypatch):
    import hibag_amd as hib
    from hibag_amd import _lib
    hib.hlaSetKernelTarget("hip")
    obj, model, _ = model_of(name)
    S = set_env(monkeypatch, pass2, None, None, None)
    m = object.__new__(hib.HlaAttrBagClass)
    m.obj, m._h = obj, R.new_model_handle(obj)
    try:
        plan = R.plan_of_handle(m.handle)
        _lib.check(_lib.lib().hibag_hip_model_finalize(m.handle))           # planning left the model unfinalized and usable
        a = R.audit(plan, model, S)
        assert not a.findings, a.findings[:5]
        assert m.stored_cells() == (plan["cell_row"][model.C] if plan["store_cells"] else 0)
        assert m.second_pass_pairs() == plan["second_pass_pairs"]
        assert m.pair_evals() == plan["pair_evals"]
        for c in range(model.C):
            assert m.engine(c) == (ENGINE_NAME[int(plan["engine"][c])], int(plan["n_step"][c])), c
        assert np.array_equal(m.mutation_table(), plan["tab"])
        G = cohort(obj, 11)
        got = m.predict_raw(G, 1, want_dosage=False, want_prob=True)["postprob"]
        p1, p2 = R.replay(a, G)
        assert same_posterior(got, p1) and same_posterior(got, p2)
        assert m.handover_faults() == 0 and m.status() == 0
    finally:
        m.close()
