"""The two ends of a structured anneal on every kernel form: what a run reports when it ends, and -- with no sweeps between
them -- where it starts.  GPU only.

Every case anneals R <= 7 replicas for 0 and for 3 sweeps, from the replica's own Philox stream and from given states, on
a form forced with the planner's options (and ``MI_K2_STATE``), with ``kernel_name()`` asserted.  The reported energies
must EQUAL (``array_equal``) tests/chain_ends_reference.py evaluated on the returned states and the model as the device
holds it: the fp64 sums in the order DESIGN.md ("Chain ends") specifies.  Forms that share a summation shape -- K2, K2p,
K2w and K2s with one wavefront on one layout; K3 and K3f -- must return the same states, energies and accepted counts;
a run of no sweeps from given states returns them.

Binary: n = 70 (degree <= 16) and n = 257 (degree 17 .. 30: five slots, a last Philox block of one slot, a last slot of one
seat) in 64-seat padded layouts; 128- and 256-seat blocks for K2w with 2 / 4 slots per step and K2s with 2 / 4 wavefronts;
a row of 70 on the runtime-width K2 (W = 80); pair-term weights; an fp64 energy model; c_pair 0, 0.4, -0.02.
Potts: n = 70 / 257, K = 2, 9, 16 on K3f (both label encodings, widths 16 and 32, with and without a threshold wavefront,
with a minimum cluster size) and on K3, K = 64 and a row of 70 on K3, R = 5 (a partly filled workgroup), holes
(``set_absent``: the padded layouts), node weights in two resolution groups.

K2p sweeps a model with pair-term weights only in runs of more than 1024 replicas: that case runs 1026 and holds the
first and last four to the reference."""
import numpy as np
import pytest

import chain_ends_cases as cc
import chain_ends_reference as ref
from scrna_seq_qannealing_clustering_amd.engine import Problem

pytestmark = pytest.mark.gpu

K2_ONLY = {"k2_pair": 2, "k2_split": 2}
BETAS = np.geomspace(0.3, 3.0, 3)


def k2(D, xs, tw=False):
    return "k_anneal_csr_rank1<%d, %d%s>" % (D, xs, ", tw" if tw else "")


# model -> [(form id, options, MI_K2_STATE, kernel name (a trailing "*": prefix), wavefronts per replica, R)]
BINARY_FORMS = {
    "b70": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 7),
            ("k2-byte-tw", K2_ONLY, "byte", k2(16, 1, True), 1, 7),
            ("k2-bit", dict(K2_ONLY, k2_tw=2), "bit", k2(16, 0), 1, 7),
            ("k2p-tw", {"k2_pair": 1}, None, "k_anneal_csr_rank1_pair<16, tw>*", 1, 7),
            ("k2p", {"k2_pair": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_pair<16>", 1, 7),
            ("k2w1-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<16, 1, tw>", 1, 7),
            ("k2s1", {"k2_split": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_split<16, 1>", 1, 7)],
    "b257": [("k2-half", K2_ONLY, None, k2(32, 2), 1, 7),
             ("k2-byte", dict(K2_ONLY, k2_tw=2), "byte", k2(32, 1), 1, 7),
             ("k2-bit-tw", K2_ONLY, "bit", k2(32, 0, True), 1, 7),
             ("k2p", {"k2_pair": 1}, None, "k_anneal_csr_rank1_pair<32>", 1, 7),
             ("k2w1-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<32, 1, tw>", 1, 7),
             ("k2s1", {"k2_split": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_split<32, 1>", 1, 7)],
    "b128": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 7),
             ("k2w2-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<16, 2, tw>", 1, 7),
             ("k2w2", {"k2_split": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_wide<16, 2>", 1, 7),
             ("k2s2", {"k2_split": 1, "k2_wide": 2}, None, "k_anneal_csr_rank1_split<16, 2>", 2, 7)],
    "b256": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 7),
             ("k2w4-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<16, 4, tw>", 1, 7),
             ("k2w4", {"k2_split": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_wide<16, 4>", 1, 7),
             ("k2s4", {"k2_split": 1, "k2_wide": 2}, None, "k_anneal_csr_rank1_split<16, 4>", 4, 7)],
    "hub70": [("k2-half", K2_ONLY, None, k2(0, 2), 1, 7),
              ("k2-byte", K2_ONLY, "byte", k2(0, 1), 1, 7),
              ("k2-bit", K2_ONLY, "bit", k2(0, 0), 1, 7)],
    "wgt": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 7),
            ("k2w1-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<16, 1, tw>", 1, 7),
            ("k2p-many", {"k2_split": 2}, None, "k_anneal_csr_rank1_pair<16*", 1, 1026)],
    "f64": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 7),
            ("k2p-tw", {"k2_pair": 1}, None, "k_anneal_csr_rank1_pair<16, tw>*", 1, 7),
            ("k2s1", {"k2_split": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_split<16, 1>", 1, 7)],
    "c0": [("k2-half", K2_ONLY, None, k2(16, 2), 1, 1),
           ("k2p-tw", {"k2_pair": 1}, None, "k_anneal_csr_rank1_pair<16, tw>*", 1, 1),
           ("k2p", {"k2_pair": 1, "k2_tw": 2}, None, "k_anneal_csr_rank1_pair<16>", 1, 1),
           ("k2w1-tw", {"k2_split": 1}, None, "k_anneal_csr_rank1_wide<16, 1, tw>", 1, 1)],
}
BINARY_IDS = ["%s-%s" % (m, f[0]) for m, forms in BINARY_FORMS.items() for f in forms]


def name_matches(got, want):
    return got.startswith(want[:-1]) if want.endswith("*") else got == want


def run_all(p, R, init, seed=11, **kw):
    """The four runs of a case: (sweeps, given) -> (states, energies, accepted)."""
    out = {}
    for sweeps in (0, 3):
        for given in (False, True):
            p.anneal(R, BETAS[:sweeps], seed, initial_states=init if given else None, **kw)
            st, en, info = p.fetch()
            out[sweeps, given] = (st, en, info["accepted"])
    return out


_BINARY_RUNS = {}


def binary_runs(case):
    """The four runs of one form of one model, computed once per session whichever test asks first."""
    if case in _BINARY_RUNS:
        return _BINARY_RUNS[case]
    mname, fid = case.split("-", 1)
    _, options, state, kernel, waves, R = next(f for f in BINARY_FORMS[mname] if f[0] == fid)
    m = cc.model(mname)
    init = np.random.RandomState(5).randint(0, 2, size=(R, m.n)).astype(np.uint8)
    energy_model = (m.val64, m.lin64, m.c64) if m.spec.f64 else None
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MI_K2_STATE", raising=False)
        if state:
            mp.setenv("MI_K2_STATE", state)
        with Problem.csr_rank1(m.rowptr, m.col, m.val, m.lin, m.c_pair, offset=0.75, order=m.spec.order, block=m.spec.block,
                               energy_model=energy_model, weights=m.weights) as p:
            assert p.n_dev == m.n_dev and np.array_equal(np.arange(m.n) if p._inv is None else p._inv, m.seats)
            for k, v in options.items():
                p.set_option(k, v)
            runs = run_all(p, R, init)
            assert name_matches(p.kernel_name(), kernel), p.kernel_name()
    _BINARY_RUNS[case] = (m, init, waves, R, runs)
    return _BINARY_RUNS[case]


@pytest.mark.parametrize("case", BINARY_IDS)
def test_binary_form_reports_the_reference_energy(case):
    m, init, waves, R, runs = binary_runs(case)
    rows = np.arange(R) if R <= 7 else np.r_[0:4, R - 4:R]
    for (sweeps, given), (st, en, accepted) in runs.items():
        assert st.shape == (R, m.n) and st.dtype == np.uint8
        want = ref.binary_energies(m.to_device(st[rows], np.uint8), *cc.binary_reference_args(m), offset=0.75,
                                   weights=m.d_weights, waves=waves)
        print(case, sweeps, given, "max |device - reference| =", np.abs(en[rows] - want).max())
        assert np.array_equal(en[rows], want), (sweeps, given)
        if sweeps == 0:
            assert accepted == 0
            if given:
                assert np.array_equal(st, init)
    if m.n > 64:
        assert runs[3, False][2] > 0 and runs[3, True][2] > 0      # (not vacuous: the chain moved)


@pytest.mark.parametrize("mname", [m for m in BINARY_FORMS])
def test_binary_forms_of_one_shape_return_the_same_run(mname):
    """K2, K2p, K2w and K2s with one wavefront on one layout, the same replicas: states, energies, accepted counts."""
    forms = [f for f in BINARY_FORMS[mname] if f[4] == 1]
    assert len(forms) >= 3
    first = binary_runs("%s-%s" % (mname, forms[0][0]))[4]
    for f in forms[1:]:
        other = binary_runs("%s-%s" % (mname, f[0]))[4]
        for key in first:                                           # (a longer run: its first replicas are this run's)
            R = len(first[key][0])
            assert np.array_equal(other[key][0][:R], first[key][0]), (f[0], key)
            assert np.array_equal(other[key][1][:R], first[key][1]), (f[0], key)
            assert other[key][2] == first[key][2] or len(other[key][0]) != R, (f[0], key)
    # more wavefronts per replica (K2s): the same chain, the energy summed per wave first
    for f in BINARY_FORMS[mname]:
        if f[4] > 1:
            other = binary_runs("%s-%s" % (mname, f[0]))[4]
            for key in first:
                assert np.array_equal(other[key][0], first[key][0]) and other[key][2] == first[key][2], (f[0], key)


# ---- Potts -----------------------------------------------------------------------------------------------------------------
def k3f(D, KM, tw):
    return "k_anneal_potts_fast<%d, %d%s>" % (D, KM, ", tw" if tw else "")


# (case id, model, K, R, minimum cluster size, [(form, options, kernel name)])
def _potts_cases():
    out = []
    for mname, D in (("p70", 16), ("p257", 16), ("p257w", 32)):
        for K in (2, 9, 16):
            KM = 8 if K <= 8 else 16
            for ms in ((0, 3) if (mname, K) in (("p70", 2), ("p257", 9), ("p257w", 16)) else (0,)):
                out.append(("%s-K%d-min%d" % (mname, K, ms), mname, K, 7, ms,
                            [("k3f-tw", {}, k3f(D, KM, True)), ("k3f", {"k2_tw": 2}, k3f(D, KM, False)),
                             ("k3", {"k3_fast": 2}, "k_anneal_potts<%d>" % D)]))
    out.append(("p257-K64", "p257", 64, 7, 0, [("k3", {}, "k_anneal_potts<16>")]))
    out.append(("phub-K9", "phub", 9, 7, 0, [("k3", {}, "k_anneal_potts<0>")]))
    out.append(("p70-K9-R5", "p70", 9, 5, 0, [("k3", {"k3_fast": 2}, "k_anneal_potts<16>"), ("k3f-tw", {}, k3f(16, 16, True))]))
    return out


POTTS_CASES = _potts_cases()


def given_labels(R, n, K):
    """Every cluster well above any minimum size used here."""
    return ((np.arange(R * n).reshape(R, n) * 7 + np.arange(R)[:, None]) % K).astype(np.uint16)


@pytest.mark.parametrize("case", POTTS_CASES, ids=[c[0] for c in POTTS_CASES])
def test_potts_forms_report_the_reference_energy(case):
    _, mname, K, R, min_size, forms = case
    m = cc.model(mname)
    init = given_labels(R, m.n, K)
    per_form = []
    for fid, options, kernel in forms:
        with Problem.potts_csr(m.rowptr, m.col, m.val, m.c_pair, m.n, K, lin_offset=-2.5, order=m.spec.order) as p:
            assert p.n_dev == m.n_dev and np.array_equal(np.arange(m.n) if p._inv is None else p._inv, m.seats)
            for k, v in options.items():
                p.set_option(k, v)
            if min_size:
                p.set_option("min_cluster_size", min_size)
            runs = run_all(p, R, init)
            assert p.kernel_name() == kernel, p.kernel_name()
        per_form.append(runs)
        for (sweeps, given), (st, en, accepted) in runs.items():
            assert st.shape == (R, m.n) and st.dtype == np.uint16 and st.max() < K
            want = ref.potts_energies(m.to_device(st, np.uint16), m.d_rowptr, m.d_col, m.d_val, m.c_pair, -2.5, K,
                                      present=m.present)
            print(case[0], fid, sweeps, given, "max |device - reference| =", np.abs(en - want).max())
            assert np.array_equal(en, want), (fid, sweeps, given)
            if sweeps == 0:
                assert accepted == 0
                if given:
                    assert np.array_equal(st, init)
        assert runs[3, False][2] > 0
    for other in per_form[1:]:                                      # K3 and K3f: the same run
        for key in per_form[0]:
            assert np.array_equal(other[key][0], per_form[0][key][0]) and np.array_equal(other[key][1], per_form[0][key][1])
            assert other[key][2] == per_form[0][key][2]


@pytest.mark.parametrize("mname,K", [("p70", 9), ("p257", 2), ("p257w", 16), ("phub", 9)])
def test_potts_node_weights_in_two_resolution_groups(mname, K):
    """Chain 2d: the integer cluster sums at the start, own / per-cluster butterflies / tot on lane 0 at the end, the
    group's pair coefficient and offset -- R = 6 replicas, three per group."""
    m = cc.model(mname)
    wq, cw, w64, c64, offset = cc.node_weights(m)
    nw = np.zeros(m.n_dev)
    nw[m.seats] = w64
    R = 6
    init = given_labels(R, m.n, K)
    betas = np.stack([BETAS, 2.0 * BETAS])
    fast = m.spec.order == "padded"
    D = {"p70": 16, "p257": 16, "p257w": 32, "phub": 0}[mname]
    forms = [("k3", {"k3_fast": 2}, "k_anneal_potts<%d, weighted>" % D)]
    if fast:
        forms += [("k3f-tw", {}, "k_anneal_potts_fast<%d, %d, tw, weighted>" % (D, 8 if K <= 8 else 16)),
                  ("k3f", {"k2_tw": 2}, "k_anneal_potts_fast<%d, %d, weighted>" % (D, 8 if K <= 8 else 16))]
    per_form = []
    for fid, options, kernel in forms:
        with Problem.potts_csr(m.rowptr, m.col, m.val, float(np.float32(c64[0])), m.n, K, lin_offset=offset[0],
                               order=m.spec.order, node_weights=(wq, cw[0], w64)) as p:
            p.set_node_weight_groups(cw, c64, offset)
            for k, v in options.items():
                p.set_option(k, v)
            runs = {}
            for sweeps in (0, 3):
                for given in (False, True):
                    p.anneal(R, betas[:, :sweeps], 13, initial_states=init if given else None)
                    st, en, info = p.fetch()
                    runs[sweeps, given] = (st, en, info["accepted"])
            assert p.kernel_name() == kernel, p.kernel_name()
        per_form.append(runs)
        for (sweeps, given), (st, en, accepted) in runs.items():
            dev = m.to_device(st, np.uint16)
            want = np.array([ref.potts_energy(dev[r], m.d_rowptr, m.d_col, m.d_val, c64[r // 3], offset[r // 3], K, nw64=nw)
                             for r in range(R)])
            print(mname, fid, sweeps, given, "max |device - reference| =", np.abs(en - want).max())
            assert np.array_equal(en, want), (fid, sweeps, given)
            if sweeps == 0 and given:
                assert np.array_equal(st, init) and accepted == 0
    for other in per_form[1:]:
        for key in per_form[0]:
            assert np.array_equal(other[key][0], per_form[0][key][0]) and np.array_equal(other[key][1], per_form[0][key][1])
            assert other[key][2] == per_form[0][key][2]
