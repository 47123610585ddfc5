"""The cases of tests/k2_state_cases.py on the planner and the oracle alone, without a GPU: every case plans -- under its
MI_K2_STATE -- to the kernel it names, the 16 forms K2 is built in are all some case's kernel, and every case is worth
running: moves are accepted, the final states are mixed, a variable with more than four neighbours inside its slot flips
(the ``rows[]`` tail of the kernel's serial loop), a weighted variable flips, a padded layout has holes and they stay 0.
Without these a device with a wrong state form could pass tests/test_gpu_k2_state_forms.py on a run that never moves."""
import numpy as np
import pytest

import k2_state_cases as kc
from scrna_seq_qannealing_clustering_amd import _lib, engine


def plan(c, monkeypatch, R=None):
    d = kc.device_model(c.model)
    monkeypatch.delenv("MI_K2_STATE", raising=False)
    if c.state:
        monkeypatch.setenv("MI_K2_STATE", c.state)
    return engine.plan_anneal(_lib.KIND_CSR_RANK1, d.rowptr, d.col, d.n_dev, c.R if R is None else R,
                              options=dict(c.options), pair_weight_slot=d.wslot)[0]


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_plans_to_its_kernel(name, monkeypatch):
    c = kc.BY_NAME[name]
    s, d = kc.MODELS[c.model], kc.device_model(c.model)
    assert plan(c, monkeypatch) == c.kernel
    # the name is what the table says of the model: the width of the device rows, the state form, the threshold wavefront
    width = int(np.diff(d.rowptr).max(initial=0))
    D = 16 if width <= 16 else 32 if width <= 32 else 64 if width <= 64 else 0
    assert D == s.D and s.W == (s.D if s.D else (width + 15) // 16 * 16)
    assert c.kernel == kc.K(s.D, kc.XS[c.state], c.tw) and c.kernel in kc.ALL_KERNELS
    assert d.n_dev <= 1024 and c.sweeps <= 6
    if c.scenario == "many":
        # more than 1024 replicas: no threshold wavefront although the option leaves it on -- up to 1024 there is one
        assert c.R > 1024 and dict(c.options).get("k2_tw") is None
        if c.state:
            assert plan(c, monkeypatch, R=1024) == kc.K(s.D, kc.XS[c.state], True)
    else:
        assert c.R <= 9
    if c.state and not c.tw and s.D in (16, 32) and c.scenario != "many":
        assert dict(c.options)["k2_tw"] == 2


def test_the_table_covers_every_form_size_and_scenario():
    assert {c.kernel for c in kc.CASES} == set(kc.ALL_KERNELS) and len(kc.ALL_KERNELS) == 16
    for state in ("byte", "bit"):
        mine = [c for c in kc.CASES if c.state == state]
        # every scenario with and without a threshold wavefront
        for scenario in kc.SCENARIOS:
            if scenario == "many":
                assert any(c.scenario == scenario and c.R > 1024 for c in mine)
                continue
            assert {c.tw for c in mine if c.scenario == scenario} == {True, False}, (state, scenario)
        # every width: D = 16 / 32 with and without, D = 64 / 0 without
        assert {(kc.MODELS[c.model].D, c.tw) for c in mine} == {(16, True), (16, False), (32, True), (32, False), (64, False), (0, False)}
        # every model, so every size and row width; the runtime-width form at W = 80 and W = 144
        assert {c.model for c in mine} == set(kc.MODELS)
        # beside a threshold wavefront (four slots' worth of thresholds a group): 1, 2, 3, 5 and 11 slots and padded layouts
        slots_tw = {(kc.device_model(c.model).n_dev + 63) // 64 for c in mine if c.tw}
        assert {1, 2, 3, 5, 11} <= slots_tw
        for order in (None, "slots", "padded"):
            assert {c.tw for c in mine if kc.MODELS[c.model].order == order} == {True, False}
        # the fp64 epilogue at every width
        assert {kc.MODELS[c.model].D for c in mine if c.scenario == "energy64"} >= {16, 32} and \
            {kc.MODELS[c.model].D for c in kc.CASES if c.scenario == "energy64"} == {16, 32, 64, 0}
    assert sorted(s.n for s in kc.MODELS.values() if not s.heavy) == sorted([1, 31, 33, 63, 64, 65, 130, 130, 130, 257, 257, 257,
                                                                             257, 257, 700, 700, 700])
    assert {s.W for s in kc.MODELS.values()} == {16, 32, 64, 80, 144}
    assert {np.sign(s.c_pair) for s in kc.MODELS.values()} == {-1.0, 0.0, 1.0}
    assert set(kc.SAME_RUN) <= set(kc.MODELS) and {kc.MODELS[m].D for m in kc.SAME_RUN} == {16, 32, 64, 0}
    for m in kc.SAME_RUN:
        forms = kc.forms_of(m)
        assert forms[0].state is None and len({c.kernel for c in forms}) == len(forms) == (5 if kc.MODELS[m].D in (16, 32) else 3)
        assert len({(c.seed, c.R, c.sweeps, c.scenario) for c in forms}) == 1


@pytest.mark.parametrize("name", sorted(kc.MODELS))
def test_model_is_what_the_table_says(name):
    s, m, d = kc.MODELS[name], kc.model(name), kc.device_model(name)
    deg = np.diff(m.rowptr)
    rows = np.repeat(np.arange(d.n_dev), np.diff(d.rowptr))
    in_slot = (rows >> 6) == (d.col >> 6)
    print("%s: n = %d (%d seats, %d holes), max degree %d, %d in-slot entries, %d variables with more than four"
          % (name, m.n, d.n_dev, len(d.holes), deg.max(initial=0), int(in_slot.sum()), len(d.heavy)))
    assert m.n == s.n + s.heavy and np.array_equal(d.val, d.val.astype(np.float32))
    if m.n > 1:
        assert (m.val < 0).any() and (m.val > 0).any()                        # couplings of both signs
        assert not np.array_equal(m.val64, m.val.astype(np.float64))          # the fp64 model is not the fp32 one widened
    if name in kc.IN_SLOT:
        assert m.order is None and len(d.heavy) > 0
        inside = np.bincount(rows[in_slot], minlength=d.n_dev)
        assert inside.max() >= (12 if name.startswith("ring") and m.n >= 31 else 5)
    if name == "mixed257":
        flagged = np.unique(rows[in_slot] >> 6)
        assert flagged.tolist() == [0, 2] and d.n_dev == 257                 # slots 1, 3 and 4 take the integer fast path
    if m.order in ("slots", "padded"):
        assert not in_slot.any()                                             # every slot takes the integer fast path
    if m.order == "padded":
        assert len(d.holes) > 0 and np.all(np.isinf(d.lin[d.holes])) and np.all(np.isfinite(d.lin[d.seats]))
        assert not np.diff(d.rowptr)[d.holes].any() and not d.lin64[d.holes].any()
    else:
        assert len(d.holes) == 0 and np.all(np.isfinite(d.lin))
    if s.heavy:
        assert m.c_pair != 0.0 and d.wslot == d.n_dev // 64 - 1 and d.wslot >= 1
        heavy_seats = d.seats[m.weights != 1]
        assert np.all(heavy_seats // 64 == d.wslot) and (m.weights > 1).sum() == s.heavy
        assert np.array_equal(d.weights[d.seats], m.weights) and np.all(d.weights[d.holes] == 1)
    else:
        assert d.wslot == -1 and d.weights is None


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_is_not_vacuous_on_the_oracle(name):
    c = kc.BY_NAME[name]
    m, d, ref = kc.model(c.model), kc.device_model(c.model), kc.reference(name)
    trail, acc = kc.replay(c)
    R = ref.states.shape[0]
    flips = trail[1:] != trail[:-1]                                           # [sweeps, R, n_dev]: a variable is proposed once a sweep
    print("%s: %s, accepted %d of %d, ones %.2f, flips of variables with > 4 in-slot neighbours %d, in the weighted slot %d"
          % (name, c.kernel, ref.accepted, ref.proposals, ref.states[:, d.seats].mean(), int(flips[:, :, d.heavy].sum()),
             int(flips[:, :, 64 * d.wslot:64 * d.wslot + 64].sum()) if d.wslot >= 0 else 0))
    # the replay IS the run (scenario "many": of its first slice)
    first = slice(0, kc.MANY_WIDTH) if c.scenario == "many" else slice(None)
    assert np.array_equal(trail[-1], ref.states[first])
    if c.scenario != "many":
        assert acc == ref.accepted == int(flips.sum())
    assert ref.proposals == R * c.sweeps * m.n
    assert 0 < ref.accepted < ref.proposals
    # neither all 0 nor all 1: over the run, and (but for the single variable) in every replica
    mine = ref.states[:, d.seats]
    assert mine.any() and not mine.all()
    if m.n > 1:
        assert np.all(mine.any(axis=1)) and not np.any(mine.all(axis=1))
    if c.model in kc.IN_SLOT:
        assert flips[:, :, d.heavy].any()
        tail = [i for i in d.heavy if flips[:, :, i].any()]
        assert len(tail) >= min(3, len(d.heavy))
    if d.wslot >= 0:
        heavy_seats = d.seats[m.weights != 1]
        assert flips[:, :, heavy_seats].any() and flips[:, :, d.seats[m.weights == 1]].any()
    if m.order == "padded":
        assert len(d.holes) > 0 and not trail[:, :, d.holes].any()
    if c.scenario == "init":
        assert np.array_equal(trail[0][:, d.seats], c.init) and c.init.any() and not c.init.all()
    if c.scenario == "offset":
        assert c.run["replica_offset"] < 2 ** 31 <= c.run["replica_offset"] + c.R - 1      # the replica ids cross 2^31
    if c.scenario == "perbeta":
        assert len(c.betas) == c.R and len(set(c.betas.tolist())) == c.R
    if c.scenario == "energy64":
        # the fp64 model's energies are told apart from the fp32 model's at the tolerance the GPU test holds them to, and
        # that tolerance is above what another summation order moves an fp64 sum of these terms by
        e64 = kc.energies64(c.model, mine)
        assert not np.allclose(e64, ref.energies, rtol=1e-12, atol=1e-9)
        terms = np.abs(m.lin64).sum() + 0.5 * np.abs(m.val64).sum() + abs(m.c64) * m.n * m.n / 2
        assert d.n_dev * np.finfo(np.float64).eps * terms < 1e-9
