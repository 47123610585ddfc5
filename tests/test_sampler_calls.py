"""What ``MI355XSampler`` asks of a ``Problem``, call by call, without a GPU: ``sampler.Problem`` is a recording stand-in
whose ``fetch`` returns states and energies that are a function of the arguments of the last ``anneal``, so a changed
argument changes the SampleSet.  Every case writes out the calls it expects (names, order, arguments with their dtypes),
the records and every ``info`` entry but the wall-clock numbers.  The cases are the single and the grouped Potts entry
with and without their options, the random remainder of partial initial states on all three model kinds, the minimum
cluster size and the empty model.  CPU only."""
import zlib

import numpy as np
import pytest

from conftest import load_fixture
from scrna_seq_qannealing_clustering_amd import models
from scrna_seq_qannealing_clustering_amd import sampler as smod
from scrna_seq_qannealing_clustering_amd.engine import layout_block_for
from scrna_seq_qannealing_clustering_amd.metrics import mean_pair_agreement
from scrna_seq_qannealing_clustering_amd.sampleset import SampleSet

K = 8
READS, SWEEPS, SEED, REPLICA_OFFSET = 5, 6, 11, 5
KERNEL_MS, KERNEL_NAME, MERGES = 2.0, "k_stand_in", 7
FP64 = "device fp64 (caller's coefficients)"
GAMMAS = (0.5, 0.8, 1.3)


# ---- the stand-in -------------------------------------------------------------------------------------------------------

def digest(*parts):
    h = 0
    for p in parts:
        if isinstance(p, np.ndarray):
            p = (str(p.dtype), p.shape, np.ascontiguousarray(p).tobytes())
        h = zlib.crc32(repr(p).encode(), h)
    return h


def run_of(anneal, n, num_cases, dtype):
    """``(states, energies, stats, key)`` the stand-in holds after ``anneal(**anneal)``: a function of every argument."""
    key = digest(*[anneal[k] for k in sorted(anneal)])
    rng = np.random.RandomState(key)
    R = anneal["num_reads"]
    states = rng.randint(0, num_cases, size=(R, n)).astype(dtype)
    energies = rng.standard_normal(R)
    stats = {"proposals": R * int(np.shape(anneal["betas"])[-1]) * n, "accepted": key % 1000, "row_bytes": 0}
    return states, energies, stats, key


def agreement_of(key, G, Rg):
    rng = np.random.RandomState(key ^ 1)
    P = Rg * (Rg - 1) // 2
    return {"ari": rng.rand(G, P), "nmi": rng.rand(G, P)}


def components_of(states):
    comps = states.astype(np.int32) * 2 + (np.arange(states.shape[1], dtype=np.int32) % 2)
    return comps, (comps.max(axis=1) + 1).astype(np.int32)


def consensus_of(G, n):
    return [{"pac": 0.25 + g, "consensus_labels": np.full(n, g, dtype=np.int64)} for g in range(G)]


def copied(v):
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, (tuple, list)):
        return type(v)(copied(x) for x in v)
    return v


class StandIn:
    """Records every call the sampler makes on ``Problem`` into ``StandIn.log`` as ``(name, arguments by name)``."""
    log = None

    def __init__(self, n, num_cases, dtype, device):
        self.n, self.num_cases, self.dtype, self.device = n, num_cases, dtype, device
        self.last = None

    @classmethod
    def note(cls, name, **kw):
        cls.log.append((name, {k: copied(v) for k, v in kw.items()}))

    @classmethod
    def potts_csr(cls, rowptr, col, val, c_pair, n, num_cases, lin_offset=0.0, device=0, order=None, energy_model=None,
                  node_weights=None):
        cls.note("potts_csr", rowptr=rowptr, col=col, val=val, c_pair=c_pair, n=n, num_cases=num_cases,
                 lin_offset=lin_offset, device=device, order=order, energy_model=energy_model, node_weights=node_weights)
        return cls(n, num_cases, np.uint16, device)

    @classmethod
    def csr_rank1(cls, rowptr, col, val, lin, c_pair, offset=0.0, device=0, order=None, energy_model=None, block=64,
                  weights=None):
        cls.note("csr_rank1", rowptr=rowptr, col=col, val=val, lin=lin, c_pair=c_pair, offset=offset, device=device,
                 order=order, energy_model=energy_model, block=block, weights=weights)
        return cls(len(rowptr) - 1, 2, np.uint8, device)

    @classmethod
    def dense(cls, Qs, offset=0.0, device=0):
        cls.note("dense", Qs=Qs, offset=offset, device=device)
        return cls(Qs.shape[0], 2, np.uint8, device)

    def __enter__(self):
        self.note("enter")
        return self

    def __exit__(self, *exc):
        self.note("exit")

    def set_node_weight_groups(self, cw, c64, offset):
        self.note("set_node_weight_groups", cw=cw, c64=c64, offset=offset)

    def set_merge_moves(self, interval, proposals=None, cq=None):
        self.note("set_merge_moves", interval=interval, proposals=proposals, cq=cq)

    def set_option(self, key, value):
        self.note("set_option", key=key, value=value)

    def anneal(self, num_reads, betas, seed, replica_offset=0, initial_states=None, resync_interval=0, sweep_offset=0,
               continue_run=False, num_sweeps=None):
        args = dict(num_reads=num_reads, betas=betas, seed=seed, replica_offset=replica_offset,
                    initial_states=initial_states, resync_interval=resync_interval, sweep_offset=sweep_offset,
                    continue_run=continue_run, num_sweeps=num_sweeps)
        self.note("anneal", **args)
        self.last = run_of(self.log[-1][1], self.n, self.num_cases, self.dtype)

    def fetch(self, states=True, energies=True):
        self.note("fetch", states=states, energies=energies)
        st, en, stats, _ = self.last
        return (st.copy() if states else None), (en.copy() if energies else None), dict(stats)

    def kernel_ms(self):
        self.note("kernel_ms")
        return KERNEL_MS

    def kernel_name(self):
        self.note("kernel_name")
        return KERNEL_NAME

    def merges_accepted(self):
        self.note("merges_accepted")
        return MERGES

    def label_agreement(self, groups=None):
        self.note("label_agreement", groups=groups)
        return agreement_of(self.last[3], groups, self.last[0].shape[0] // groups)

    def components(self):
        self.note("components")
        return components_of(self.last[0])


@pytest.fixture
def log(monkeypatch):
    calls = []
    monkeypatch.setattr(StandIn, "log", calls)
    monkeypatch.setattr(smod, "Problem", StandIn)
    monkeypatch.setattr(smod._lib, "load", lambda: None)

    def consensus_info(prob, G, model, num_reads):
        StandIn.note("consensus_info", prob_is_stand_in=isinstance(prob, StandIn), G=G, model=model, num_reads=num_reads)
        return consensus_of(G, model.num_variables)

    def energy_dense_f64(Qs, X, offset=0.0, device=0):
        StandIn.note("energy_dense_f64", Qs=Qs, X=X, offset=offset, device=device)
        Xf = np.asarray(X, dtype=np.float64)
        return np.einsum("ri,ri->r", Xf @ Qs, Xf) + offset

    monkeypatch.setattr(smod, "_consensus_info", consensus_info)
    monkeypatch.setattr(smod, "energy_dense_f64", energy_dense_f64)
    return calls


def sampler():
    return smod.MI355XSampler(device=0, replica_offset=REPLICA_OFFSET)


# ---- comparing -----------------------------------------------------------------------------------------------------------

def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.array_equal(a, b))
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, models.PottsModel) or isinstance(b, models.PottsModel):
        return a is b
    return type(a) is type(b) and a == b


def assert_calls(got, want):
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert set(a) == set(b), name
        for k in b:
            assert same(a[k], b[k]), (name, k, a[k], b[k])


def assert_info(info, want, clock=("timing",)):
    """Every key and value of ``info`` but the wall-clock numbers, which sit at ``clock`` (a path of keys)."""
    assert set(info) == set(want)
    for k in want:
        if k == clock[0]:
            continue
        assert same(info[k], want[k]), (k, info[k], want[k])
    got_t, want_t = info, want
    for k in clock:
        got_t, want_t = got_t[k], want_t[k]
        assert set(got_t) == set(want_t), k
        for j in want_t:
            if j not in ("upload_s", "anneal_s", "timing"):
                assert same(got_t[j], want_t[j]), (k, j)
    for j in ("upload_s", "anneal_s"):
        assert isinstance(got_t[j], float) and got_t[j] >= 0.0


def assert_records(ss, states, energies, variables, vartype):
    want = SampleSet(states, energies, variables, vartype)
    assert ss.vartype == vartype and ss.variables == list(variables)
    assert ss.record.dtype == want.record.dtype
    for f in ("sample", "energy", "num_occurrences"):
        assert np.array_equal(ss.record[f], want.record[f]), f


# ---- the expected calls, written out -------------------------------------------------------------------------------------

CLOCK = {"upload_s": 0.0, "anneal_s": 0.0}


def graph(name="blobs"):
    return load_fixture(name).graph()


def potts_csr_call(m, node_weights):
    return ("potts_csr", dict(rowptr=m.rowptr, col=m.col, val=m.val.astype(np.float32), c_pair=float(np.float32(m.c_pair)),
                              n=m.num_variables, num_cases=m.num_cases, lin_offset=m.lin_offset, device=0, order="padded",
                              energy_model=(m.val, m.c_pair), node_weights=node_weights))


def anneal_call(num_reads, betas, initial_states=None, resync_interval=0):
    return ("anneal", dict(num_reads=num_reads, betas=betas, seed=SEED, replica_offset=REPLICA_OFFSET,
                           initial_states=initial_states, resync_interval=resync_interval, sweep_offset=0,
                           continue_run=False, num_sweeps=None))


FETCH = ("fetch", dict(states=True, energies=True))
FETCH_STATES = ("fetch", dict(states=True, energies=False))
NO_SWEEPS = np.zeros(0, dtype=np.float64)


def potts_betas(m, beta_range=None):
    rng = smod.default_potts_beta_range(m) if beta_range is None else beta_range
    return models.make_beta_schedule(SWEEPS, rng), [float(rng[0]), float(rng[1])]


def single_info(m, beta_range, num_reads, stats, ignored=()):
    return {"beta_range": beta_range, "beta_schedule_type": "geometric", "seed": SEED, "num_sweeps": SWEEPS,
            "num_reads": num_reads, "kernel": "potts_csr", "device": 0,
            "timing": dict(CLOCK, kernel_ms=KERNEL_MS), "updates_per_s": stats["proposals"] / (KERNEL_MS * 1e-3),
            "accepted": stats["accepted"], "proposals": stats["proposals"], "energy_evaluation": FP64,
            "ignored_kwargs": list(ignored)}


def option_info(m, key, G, g, num_reads, states, energies):
    """The entries ``merge_interval``, ``stability``, ``consensus`` and ``split_disconnected`` add for group g of G."""
    rows = slice(g * num_reads, (g + 1) * num_reads)
    agree = agreement_of(key, G, num_reads)
    stab, stab_nmi = mean_pair_agreement(agree["ari"][g], agree["nmi"][g])
    info = {"merges_accepted": MERGES, "stability": stab, "stability_nmi": stab_nmi}
    info.update(consensus_of(G, m.num_variables)[g])
    info.update(smod._split_info(m, states[rows], energies[rows], components_of(states)[0][rows]))
    return info


# ---- sample_dqm ----------------------------------------------------------------------------------------------------------

def test_sample_dqm_plain(log):
    m = models.build_modularity_potts(graph(), 1.0, K)
    n = m.num_variables
    betas, beta_range = potts_betas(m)
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, label="a run")
    run = anneal_call(READS, betas)
    assert_calls(log, [potts_csr_call(m, models.potts_node_weights(m)), ("enter", {}), run, FETCH, ("kernel_ms", {}),
                       ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    assert stats["proposals"] == READS * SWEEPS * n
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    assert_info(ss.info, single_info(m, beta_range, READS, stats, ignored=["label"]))


def test_sample_dqm_every_option(log):
    m = models.build_modularity_potts(graph("noisy_circles"), 0.8, K)
    n = m.num_variables
    betas, beta_range = potts_betas(m, (0.3, 7.0))
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, beta_range=(0.3, 7.0), merge_interval=3,
                              stability=True, consensus=True, split_disconnected=True)
    run = anneal_call(READS, betas)
    assert_calls(log, [
        potts_csr_call(m, models.potts_node_weights(m)), ("enter", {}),
        ("set_merge_moves", dict(interval=3, proposals=None, cq=models.potts_merge_coefficients(m))),
        run, FETCH, ("kernel_ms", {}), ("merges_accepted", {}), ("label_agreement", dict(groups=1)),
        ("consensus_info", dict(prob_is_stand_in=True, G=1, model=m, num_reads=READS)), ("components", {}), ("exit", {})])
    states, energies, stats, key = run_of(run[1], n, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    want = single_info(m, beta_range, READS, stats)
    want.update(option_info(m, key, 1, 0, READS, states, energies))
    assert_info(ss.info, want)


def test_sample_dqm_merge_proposals_and_one_read(log):
    """``merge_proposals`` reaches ``set_merge_moves``; one read has no pair of reads, so no agreement call is made."""
    m = models.build_modularity_potts(graph(), 1.0, K)
    betas, beta_range = potts_betas(m)
    ss = sampler().sample_dqm(m, num_reads=1, num_sweeps=SWEEPS, seed=SEED, merge_interval=2, merge_proposals=9,
                              stability=True)
    run = anneal_call(1, betas)
    assert_calls(log, [
        potts_csr_call(m, models.potts_node_weights(m)), ("enter", {}),
        ("set_merge_moves", dict(interval=2, proposals=9, cq=models.potts_merge_coefficients(m))),
        run, FETCH, ("kernel_ms", {}), ("merges_accepted", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], m.num_variables, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    want = single_info(m, beta_range, 1, stats)
    want.update(merges_accepted=MERGES, stability=None, stability_nmi=None)
    assert_info(ss.info, want)


def test_sample_dqm_partial_initial_states(log):
    """Two given rows of five reads: the other three start from the device's random rows (a zero-sweep anneal first)."""
    m = models.build_modularity_potts(graph(), 1.0, K)
    n = m.num_variables
    betas, beta_range = potts_betas(m)
    given = np.random.RandomState(2).randint(0, K, size=(2, n))                     # (int64, as a caller has them)
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, initial_states=given)
    first = anneal_call(READS, NO_SWEEPS)
    init = run_of(first[1], n, K, np.uint16)[0]
    init[:2] = given
    run = anneal_call(READS, betas, init)
    assert_calls(log, [potts_csr_call(m, models.potts_node_weights(m)), ("enter", {}), first, FETCH_STATES, run, FETCH,
                       ("kernel_ms", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    assert_info(ss.info, single_info(m, beta_range, READS, stats))


@pytest.mark.parametrize("from_keyword", [True, False])
def test_sample_dqm_min_cluster_size(log, from_keyword):
    """The CQM's minimum cluster size, from the keyword or from the model's info: random rows from a zero-sweep anneal,
    the repair, ``set_option``, then the anneal from the repaired rows."""
    m = models.build_cqm_potts(graph(), K, 20)
    n = m.num_variables
    betas, beta_range = potts_betas(m)
    kw = dict(min_cluster_size=25) if from_keyword else {}
    size = 25 if from_keyword else 20
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, **kw)
    first = anneal_call(READS, NO_SWEEPS)
    init = smod._make_feasible(run_of(first[1], n, K, np.uint16)[0], K, size)
    assert init.dtype == np.uint16 and all(np.bincount(r, minlength=K).min() >= size for r in init)
    run = anneal_call(READS, betas, init)
    assert_calls(log, [potts_csr_call(m, None), ("enter", {}), first, FETCH_STATES,
                       ("set_option", dict(key="min_cluster_size", value=size)), run, FETCH, ("kernel_ms", {}),
                       ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    assert_info(ss.info, single_info(m, beta_range, READS, stats))


def test_sample_dqm_min_cluster_size_with_all_rows_given(log):
    """All rows given: no zero-sweep anneal, the repair works on a uint16 copy and leaves the caller's array alone."""
    m = models.build_cqm_potts(graph(), K, 20)
    n = m.num_variables
    betas, beta_range = potts_betas(m)
    given = np.zeros((READS, n), dtype=np.int64)
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, initial_states=given)
    assert not given.any()
    init = smod._make_feasible(np.zeros((READS, n), dtype=np.uint16), K, 20)
    run = anneal_call(READS, betas, init)
    assert_calls(log, [potts_csr_call(m, None), ("enter", {}), ("set_option", dict(key="min_cluster_size", value=20)),
                       run, FETCH, ("kernel_ms", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    assert_info(ss.info, single_info(m, beta_range, READS, stats))


def test_sample_dqm_without_node_weights(log):
    """``build_dqm_potts`` has no node weights: none reach ``potts_csr``, and the merge coefficient is the library's own."""
    m = models.build_dqm_potts(graph(), K, 0.005)
    betas, beta_range = potts_betas(m)
    ss = sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, merge_interval=2)
    run = anneal_call(READS, betas)
    assert_calls(log, [potts_csr_call(m, None), ("enter", {}),
                       ("set_merge_moves", dict(interval=2, proposals=None, cq=None)), run, FETCH, ("kernel_ms", {}),
                       ("merges_accepted", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], m.num_variables, K, np.uint16)
    assert_records(ss, states.astype(np.int32), energies, m.variables, "DISCRETE")
    want = single_info(m, beta_range, READS, stats)
    want["merges_accepted"] = MERGES
    assert_info(ss.info, want)


def test_sample_dqm_empty_model(log):
    m = models.PottsModel([], 4, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0.0, np.zeros(0))
    ss = sampler().sample_dqm(m, num_reads=READS, label="nothing")
    assert log == []
    assert_records(ss, np.zeros((0, 0), dtype=np.int32), np.zeros(0), [], "DISCRETE")
    assert ss.info == {"ignored_kwargs": ["label"]}


# ---- sample_dqm_many -----------------------------------------------------------------------------------------------------

def batch_info(G, stats):
    return {"groups": G, "kernel_ms": KERNEL_MS, "kernel_name": KERNEL_NAME, "accepted": stats["accepted"],
            "proposals": stats["proposals"], "updates_per_s": stats["proposals"] / (KERNEL_MS * 1e-3), "timing": dict(CLOCK)}


def many_info(beta_range, num_reads, batch, ignored=()):
    return {"beta_range": beta_range, "beta_schedule_type": "geometric", "seed": SEED, "num_sweeps": SWEEPS,
            "num_reads": num_reads, "kernel": "potts_csr", "device": 0, "batch": batch, "energy_evaluation": FP64,
            "ignored_kwargs": list(ignored)}


def test_sample_dqm_many_three_resolutions_every_option(log):
    """A [3, 2] ``beta_range``, two given rows of four reads per model: the remainder is group 0's random rows, the four
    rows are tiled to every group."""
    ms = models.build_modularity_sweep(graph("noisy_circles"), GAMMAS, K)
    n, G, reads = ms[0].num_variables, 3, 4
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(ms)
    ranges = [(0.2, 5.0), (0.3, 6.0), (0.4, 7.0)]
    scheds = [potts_betas(m, r) for m, r in zip(ms, ranges)]
    betas = np.stack([b for b, _ in scheds])
    given = np.random.RandomState(3).randint(0, K, size=(2, n))
    out = sampler().sample_dqm_many(ms, num_reads=reads, num_sweeps=SWEEPS, seed=SEED, beta_range=ranges,
                                    initial_states=given, merge_interval=3, stability=True, consensus=True,
                                    split_disconnected=True, label="a sweep")
    first = anneal_call(reads * G, NO_SWEEPS)
    init = run_of(first[1], n, K, np.uint16)[0][:reads]
    init[:2] = given
    run = anneal_call(reads * G, betas, np.tile(init, (G, 1)))
    assert_calls(log, [
        potts_csr_call(ms[0], (wq, cw[0], w64)), ("enter", {}),
        ("set_node_weight_groups", dict(cw=cw, c64=c64, offset=offset)),
        ("set_merge_moves", dict(interval=3, proposals=None, cq=models.potts_merge_coefficients(ms))),
        first, FETCH_STATES, run, FETCH, ("kernel_ms", {}), ("kernel_name", {}), ("merges_accepted", {}),
        ("label_agreement", dict(groups=G)),
        ("consensus_info", dict(prob_is_stand_in=True, G=G, model=ms[0], num_reads=reads)), ("components", {}),
        ("exit", {})])
    states, energies, stats, key = run_of(run[1], n, K, np.uint16)
    assert stats["proposals"] == reads * G * SWEEPS * n
    assert len(out) == G
    for g, (m, ss) in enumerate(zip(ms, out)):
        rows = slice(g * reads, (g + 1) * reads)
        assert_records(ss, states[rows].astype(np.int32), energies[rows], m.variables, "DISCRETE")
        want = many_info(scheds[g][1], reads, batch_info(G, stats), ignored=["label"])
        want.update(option_info(m, key, G, g, reads, states, energies))
        assert_info(ss.info, want, clock=("batch", "timing"))
        assert ss.info["batch"] is out[0].info["batch"]


@pytest.mark.parametrize("rows_given", [False, True])
def test_sample_dqm_many_one_model_still_sets_one_group(log, rows_given):
    m = models.build_modularity_potts(graph(), 1.0, K)
    n = m.num_variables
    wq, cw, w64, c64, offset = models.potts_node_weight_groups([m])
    betas, beta_range = potts_betas(m)
    given = np.random.RandomState(6).randint(0, K, size=(READS, n))                # (int64: tiled once, as uint16)
    kw = dict(initial_states=given) if rows_given else dict(num_reads=READS)
    out = sampler().sample_dqm_many([m], num_sweeps=SWEEPS, seed=SEED, **kw)
    run = anneal_call(READS, betas[None, :], given.astype(np.uint16) if rows_given else None)
    assert cw.shape == (1, n) and c64.shape == (1,) and offset.shape == (1,)
    assert_calls(log, [potts_csr_call(m, (wq, cw[0], w64)), ("enter", {}),
                       ("set_node_weight_groups", dict(cw=cw, c64=c64, offset=offset)), run, FETCH, ("kernel_ms", {}),
                       ("kernel_name", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    assert len(out) == 1
    assert_records(out[0], states.astype(np.int32), energies, m.variables, "DISCRETE")
    assert_info(out[0].info, many_info(beta_range, READS, batch_info(1, stats)), clock=("batch", "timing"))


def test_sample_dqm_many_all_rows_given_are_tiled_as_uint16(log):
    ms = models.build_modularity_sweep(graph(), GAMMAS[:2], K)
    n = ms[0].num_variables
    wq, cw, w64, c64, offset = models.potts_node_weight_groups(ms)
    scheds = [potts_betas(m) for m in ms]
    given = np.random.RandomState(4).randint(0, K, size=(3, n))
    out = sampler().sample_dqm_many(ms, num_sweeps=SWEEPS, seed=SEED, initial_states=given)      # (3 reads: the rows given)
    run = anneal_call(6, np.stack([b for b, _ in scheds]), np.tile(given.astype(np.uint16), (2, 1)))
    assert_calls(log, [potts_csr_call(ms[0], (wq, cw[0], w64)), ("enter", {}),
                       ("set_node_weight_groups", dict(cw=cw, c64=c64, offset=offset)), run, FETCH, ("kernel_ms", {}),
                       ("kernel_name", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, K, np.uint16)
    for g, (m, ss) in enumerate(zip(ms, out)):
        assert_records(ss, states[3 * g:3 * g + 3].astype(np.int32), energies[3 * g:3 * g + 3], m.variables, "DISCRETE")
        assert_info(ss.info, many_info(scheds[g][1], 3, batch_info(2, stats)), clock=("batch", "timing"))


# ---- sample_qubo ---------------------------------------------------------------------------------------------------------

def binary_info(m, kernel, beta_range, stats, diff, ignored=()):
    return {"beta_range": beta_range, "beta_schedule_type": "geometric", "seed": SEED, "num_sweeps": SWEEPS,
            "num_reads": READS, "kernel": kernel, "device": 0, "timing": dict(CLOCK, kernel_ms=KERNEL_MS),
            "updates_per_s": stats["proposals"] / (KERNEL_MS * 1e-3), "accepted": stats["accepted"],
            "proposals": stats["proposals"], "energy_evaluation": FP64, "device_energy_max_abs_diff": diff,
            "ignored_kwargs": list(ignored)}


def binary_case(kernel):
    m = models.build_bqm_qubo(graph(), 0.05)
    n = m.num_variables
    rng = smod.default_beta_range(m)
    betas = models.make_beta_schedule(SWEEPS, rng)
    given = np.random.RandomState(5).randint(0, 2, size=(2, n))
    ss = sampler().sample_qubo(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, initial_states=given, kernel=kernel,
                               resync_interval=4, return_embedding=True)
    first = anneal_call(READS, NO_SWEEPS)
    init = run_of(first[1], n, 2, np.uint8)[0]
    init[:2] = given
    run = anneal_call(READS, betas, init, resync_interval=4)
    return m, ss, first, run, [float(rng[0]), float(rng[1])]


def test_sample_qubo_partial_initial_states_csr(log):
    m, ss, first, run, beta_range = binary_case("csr")
    n = m.num_variables
    max_deg = int(np.diff(m.rowptr).max())
    assert_calls(log, [
        ("csr_rank1", dict(rowptr=m.rowptr, col=m.col, val=m.val.astype(np.float32), lin=m.lin.astype(np.float32),
                           c_pair=float(np.float32(m.c_pair)), offset=m.offset, device=0, order="padded",
                           energy_model=(m.val, m.lin, m.c_pair), block=layout_block_for(n, READS, max_deg),
                           weights=None)),
        ("enter", {}), first, FETCH_STATES, run, FETCH, ("kernel_ms", {}), ("exit", {})])
    states, energies, stats, _ = run_of(run[1], n, 2, np.uint8)
    assert_records(ss, states.astype(np.int8), energies, m.variables, "BINARY")
    want = binary_info(m, "csr_rank1", beta_range, stats, 0.0, ignored=["return_embedding"])
    want["embedding_context"] = {"embedding": {}}
    assert_info(ss.info, want)


def test_sample_qubo_partial_initial_states_dense(log):
    m, ss, first, run, beta_range = binary_case("dense")
    n = m.num_variables
    dense64 = m.dense_Qs()
    states, dev_energy, stats, _ = run_of(run[1], n, 2, np.uint8)
    assert_calls(log, [
        ("dense", dict(Qs=np.ascontiguousarray(dense64.astype(np.float32)), offset=m.offset, device=0)),
        ("enter", {}), first, FETCH_STATES, run, FETCH, ("kernel_ms", {}), ("exit", {}),
        ("energy_dense_f64", dict(Qs=dense64, X=states, offset=m.offset, device=0))])
    Xf = states.astype(np.float64)
    energies = np.einsum("ri,ri->r", Xf @ dense64, Xf) + m.offset
    assert_records(ss, states.astype(np.int8), energies, m.variables, "BINARY")
    want = binary_info(m, "dense", beta_range, stats, float(np.max(np.abs(dev_energy - energies))),
                       ignored=["return_embedding"])
    want["embedding_context"] = {"embedding": {}}
    assert_info(ss.info, want)


def test_sample_qubo_async_yields_once_after_the_enqueued_anneal(log):
    """The generator behind ``sample_qubo_async``: when the call returns the anneal is enqueued and nothing is fetched."""
    m = models.build_bqm_qubo(graph(), 0.05)
    betas = models.make_beta_schedule(SWEEPS, smod.default_beta_range(m))
    pending = sampler().sample_qubo_async(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED)
    assert [name for name, _ in log] == ["csr_rank1", "enter", "anneal"]
    ss = pending.result()
    assert [name for name, _ in log] == ["csr_rank1", "enter", "anneal", "fetch", "kernel_ms", "exit"]
    run = anneal_call(READS, betas)
    assert_calls(log[2:3], [run])
    states, energies, _, _ = run_of(run[1], m.num_variables, 2, np.uint8)
    assert_records(ss, states.astype(np.int8), energies, m.variables, "BINARY")


# ---- the refusals this file pins that the two Potts entries did not share before ------------------------------------------
# (the two tests below are the only ones here that do not pass on the sampler as it was before the two entries shared one
# routine: they state its two deliberate behaviour changes)

@pytest.mark.parametrize("many", [False, True])
def test_num_reads_below_one_is_refused_before_any_gpu_work(log, many):
    m = models.build_modularity_potts(graph(), 1.0, K)
    s = sampler()
    with pytest.raises(ValueError, match="'num_reads' should be a positive integer"):
        s.sample_dqm_many([m], num_reads=0, num_sweeps=SWEEPS) if many else s.sample_dqm(m, num_reads=0, num_sweeps=SWEEPS)
    assert log == []


def test_min_cluster_size_that_cannot_fit_is_refused_before_any_gpu_work(log):
    m = models.build_cqm_potts(graph(), K, 20)
    n = m.num_variables
    with pytest.raises(ValueError, match="min_cluster_size %d x %d clusters exceeds the %d variables" % (n, K, n)):
        sampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, min_cluster_size=n)
    assert log == []
