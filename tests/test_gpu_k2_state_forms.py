"""Every form of K2 (k_anneal_csr_rank1<D, XS, TW>: D = 16 / 32 / 64 / runtime width, half / byte / bit state, with and
without a threshold wavefront) against the oracle at small sizes.  GPU only.

The library keeps the half form up to 4608 variables, so the byte and bit forms -- their packed neighbour words, gathers
(ds_read_u8; ds_read_b32 + v_bfe_i32), field arithmetic, write-back of an accepted flip, slot masks and fp64 epilogue
branches -- run nowhere else in the suite but on three sparse-ring models beside a threshold wavefront.  ``MI_K2_STATE``,
read when a model is created, forces them at any size: the cases of tests/k2_state_cases.py (tests/test_k2_state_cases.py
shows without a GPU that each plans to its kernel and moves on the oracle) run here with the kernel name asserted, states
and accepted counts bit-equal to oracle/sa_oracle.c on the same renumbered / padded model, exact proposal counts, energies
to rtol = atol = 1e-9 of the oracle's (with an fp64 energy model: to rtol = 1e-12, atol = 1e-9 of the host's fp64 sum), and
``best()`` consistent with ``fetch()``.  The forms of one model and seed must also return the same run as each other and
as the unforced half form.

D = 32 / 64 / the runtime width are pinned by this parity only: tests/test_gpu_chain_stationarity.py holds the byte and
bit forms to Boltzmann statistics at D = 16 (a row of 17 neighbours needs n = 18, beyond enumeration for a binary model).

Measured on an MI355X: 2.9 s for the file (88 tests; 1.6 s of it the first test's device start-up, 0.5 s the first
renumbered model), 0.01 s per case."""
import numpy as np
import pytest

import k2_state_cases as kc
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu


def problem(c, monkeypatch):
    """The case's model on the device, created under the case's MI_K2_STATE, the case's options set."""
    m, d = kc.model(c.model), kc.device_model(c.model)
    monkeypatch.delenv("MI_K2_STATE", raising=False)
    if c.state:
        monkeypatch.setenv("MI_K2_STATE", c.state)
    energy_model = (m.val64, m.lin64, m.c64) if c.scenario == "energy64" else None
    p = Problem.csr_rank1(m.rowptr, m.col, m.val, m.lin, m.c_pair, order=m.order, energy_model=energy_model, weights=m.weights)
    # the layout the oracle ran on is the one the problem took
    assert p.n == m.n and p.n_dev == d.n_dev
    assert np.array_equal(np.arange(m.n) if p._inv is None else p._inv, d.seats)
    for k, v in c.options:
        p.set_option(k, v)
    return p


def run(p, c):
    """The case's run: states (caller's order), energies, proposals and accepted moves of the whole run, the kernel."""
    kw = dict(c.run)
    if c.scenario == "split":                    # a run continued in two pieces
        cut = c.sweeps // 2
        p.anneal(c.R, c.betas[:cut], c.seed)
        first = p.fetch(states=False, energies=False)[2]
        name = p.kernel_name()
        p.anneal(c.R, c.betas[cut:], c.seed, continue_run=True, sweep_offset=cut)
        assert p.kernel_name() == name
        st, en, info = p.fetch()
        return st, en, first["proposals"] + info["proposals"], first["accepted"] + info["accepted"], name
    p.anneal(c.R, c.betas, c.seed, initial_states=c.init, **kw)
    st, en, info = p.fetch()
    return st, en, info["proposals"], info["accepted"], p.kernel_name()


def check_best(p, st, en):
    idx, e_best, _, s_best = p.best()
    assert en[idx] == en.min() and e_best == pytest.approx(en[idx], rel=1e-12) and np.array_equal(s_best, st[idx])


@pytest.mark.parametrize("name", kc.NAMES)
def test_k2_form_against_the_oracle(name, monkeypatch):
    c = kc.BY_NAME[name]
    d, ref = kc.device_model(c.model), kc.reference(name)
    with problem(c, monkeypatch) as p:
        st, en, proposals, accepted, kernel = run(p, c)
        assert kernel == c.kernel, kernel
        check_best(p, st, en)
    assert st.shape == (c.R, kc.model(c.model).n) and st.dtype == np.uint8
    if c.scenario == "many":
        # more replicas than the oracle runs in milliseconds: three slices of them (their ids are their positions)
        rows = np.concatenate([np.arange(lo, lo + kc.MANY_WIDTH) for lo in kc.MANY_PICKS])
        assert np.array_equal(st[rows], ref.states[:, d.seats])
        assert np.allclose(en[rows], ref.energies, rtol=1e-9, atol=1e-9)
        assert proposals == c.R * c.sweeps * st.shape[1] and 0 < accepted < proposals
        return
    assert np.array_equal(st, ref.states[:, d.seats])
    assert accepted == ref.accepted and proposals == ref.proposals
    if c.scenario == "energy64":
        assert np.allclose(en, kc.energies64(c.model, st), rtol=1e-12, atol=1e-9)
    else:
        assert np.allclose(en, ref.energies, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("model", kc.SAME_RUN + ("ring130-many",))
def test_state_forms_return_the_same_run(model, monkeypatch):
    """One model and seed on every form built for its width -- half (MI_K2_STATE unset), byte, bit, the latter two with and
    without a threshold wavefront: identical states, energies and counts, equal to the oracle's."""
    if model.endswith("-many"):
        forms = [c for c in kc.CASES if c.scenario == "many"]
    else:
        forms = kc.forms_of(model)
    assert forms[0].state is None
    runs = []
    for c in forms:
        with problem(c, monkeypatch) as p:
            out = run(p, c)
            check_best(p, out[0], out[1])
        assert out[4] == c.kernel, out[4]
        runs.append(out)
    assert len({r[4] for r in runs}) == len(forms)
    st, en, proposals, accepted, _ = runs[0]
    for other in runs[1:]:
        assert np.array_equal(other[0], st) and np.array_equal(other[1], en) and other[2:4] == (proposals, accepted)
    if not model.endswith("-many"):
        d, ref = kc.device_model(forms[0].model), kc.reference(forms[0])
        assert np.array_equal(st, ref.states[:, d.seats]) and (proposals, accepted) == (ref.proposals, ref.accepted)
        assert np.allclose(en, ref.energies, rtol=1e-9, atol=1e-9)


def test_given_states_of_a_padded_model_and_zero_sweeps(monkeypatch):
    """Given initial states on a padded layout (holes between the seats the caller's states go to), and a run of no sweeps:
    the states come back as given, with the energies the oracle gives them."""
    for state in ("byte", "bit"):
        for tw in (True, False):
            c = kc.make_case("deg16_257", state, tw, "init")
            d = kc.device_model(c.model)
            ost, oen, (_, oacc) = kc.oracle(c, init_dev=kc.init_dev(c))
            o0 = kc.oracle(c, betas=c.betas[:0], init_dev=kc.init_dev(c))
            with problem(c, monkeypatch) as p:
                st, en, proposals, accepted, kernel = run(p, c)
                assert kernel == c.kernel
                p.anneal(c.R, c.betas[:0], c.seed, initial_states=c.init)
                s0, e0, _ = p.fetch()
            assert np.array_equal(st, ost[:, d.seats]) and accepted == oacc and np.allclose(en, oen, rtol=1e-9, atol=1e-9)
            assert np.array_equal(s0, c.init) and np.array_equal(o0[0][:, d.seats], c.init)
            assert np.allclose(e0, o0[1], rtol=1e-9, atol=1e-9)
