"""The promise of ``MI355XSampler.sample_dqm_many`` on the device, with every option on: the SampleSet of model g equals
``sample_dqm(models[g], **kwargs)`` -- records bit for bit and every ``info`` entry the two entries share -- for three
resolutions and for a single model; and ``sample_dqm`` with a minimum cluster size equals the run written out on
``Problem.potts_csr``.  GPU only."""
import numpy as np
import pytest

from conftest import load_fixture
from scrna_seq_qannealing_clustering_amd import MI355XSampler, models
from scrna_seq_qannealing_clustering_amd.engine import Problem
from scrna_seq_qannealing_clustering_amd.sampler import _make_feasible, default_potts_beta_range
from scrna_seq_qannealing_clustering_amd.sampleset import SampleSet

pytestmark = pytest.mark.gpu

K, READS, SWEEPS, SEED = 8, 6, 40, 3
GAMMAS = (0.5, 0.8, 1.3)
# what only one of the two entries reports, or reports per launch: the launch's wall-clock and kernel time, and the move
# counts (top-level from sample_dqm, under "batch" and over all groups from sample_dqm_many)
SINGLE_ONLY = {"timing", "updates_per_s", "accepted", "proposals"}
MANY_ONLY = {"batch"}


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.array_equal(a, b))
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def kwargs(n):
    given = np.random.RandomState(7).randint(0, K, size=(2, n))
    return dict(num_reads=READS, num_sweeps=SWEEPS, seed=SEED, merge_interval=10, stability=True, consensus=True,
                split_disconnected=True, initial_states=given)


def assert_group_equals_single(many, single, groups):
    for f in ("sample", "energy", "num_occurrences"):
        assert np.array_equal(many.record[f], single.record[f]), f
    assert many.variables == single.variables and many.vartype == single.vartype
    assert set(many.info) - MANY_ONLY == set(single.info) - SINGLE_ONLY
    assert MANY_ONLY <= set(many.info) and SINGLE_ONLY <= set(single.info)
    for k in set(single.info) - SINGLE_ONLY:
        if k == "merges_accepted" and groups > 1:
            continue                                   # (all groups together, like "batch": see the caller)
        assert same(many.info[k], single.info[k]), (k, many.info[k], single.info[k])
    for k in ("stability", "stability_nmi", "pac", "edge_cooccurrence", "consensus_labels", "cell_confidence",
              "split_labels", "split_num_clusters", "split_energy", "merges_accepted"):
        assert k in single.info, k


def test_every_group_equals_its_single_run():
    G = load_fixture("noisy_circles").graph()
    ms = models.build_modularity_sweep(G, GAMMAS, K)
    kw = kwargs(ms[0].num_variables)
    s = MI355XSampler()
    many = s.sample_dqm_many(ms, **kw)
    singles = [s.sample_dqm(m, **kw) for m in ms]
    assert len(many) == len(ms)
    for ss, one in zip(many, singles):
        assert_group_equals_single(ss, one, len(ms))
        assert ss.info["batch"] is many[0].info["batch"] and ss.info["batch"]["groups"] == len(ms)
    assert many[0].info["batch"]["accepted"] == sum(one.info["accepted"] for one in singles) > 0
    assert many[0].info["batch"]["proposals"] == sum(one.info["proposals"] for one in singles)
    assert many[0].info["merges_accepted"] == sum(one.info["merges_accepted"] for one in singles)


def test_one_model_through_the_grouped_entry_equals_the_single_run():
    m = models.build_modularity_potts(load_fixture("noisy_circles").graph(), 0.8, K)
    kw = kwargs(m.num_variables)
    s = MI355XSampler()
    many = s.sample_dqm_many([m], **kw)
    one = s.sample_dqm(m, **kw)
    assert len(many) == 1
    assert_group_equals_single(many[0], one, 1)
    assert many[0].info["batch"]["groups"] == 1
    assert many[0].info["batch"]["accepted"] == one.info["accepted"] > 0
    assert many[0].info["batch"]["proposals"] == one.info["proposals"]


def test_min_cluster_size_equals_the_run_written_out():
    """Random rows from a zero-sweep anneal, the repair, the option, the anneal from the repaired rows: one seed."""
    m = models.build_cqm_potts(load_fixture("noisy_circles").graph(), 4, 20)
    n = m.num_variables
    ss = MI355XSampler().sample_dqm(m, num_reads=READS, num_sweeps=SWEEPS, seed=SEED, min_cluster_size=20)
    betas = models.make_beta_schedule(SWEEPS, default_potts_beta_range(m))
    with Problem.potts_csr(m.rowptr, m.col, m.val.astype(np.float32), float(np.float32(m.c_pair)), n, 4,
                           lin_offset=m.lin_offset, order="padded", energy_model=(m.val, m.c_pair)) as p:
        p.anneal(READS, betas[:0], SEED)
        rnd, _, _ = p.fetch(energies=False)
        init = _make_feasible(rnd.copy(), 4, 20)
        p.set_option("min_cluster_size", 20)
        p.anneal(READS, betas, SEED, initial_states=init)
        lab, en, stats = p.fetch()
    assert min(np.bincount(row, minlength=4).min() for row in lab) >= 20
    want = SampleSet(lab.astype(np.int32), en, m.variables, "DISCRETE")
    for f in ("sample", "energy", "num_occurrences"):
        assert np.array_equal(ss.record[f], want.record[f]), f
    assert ss.info["accepted"] == stats["accepted"] and ss.info["num_reads"] == READS and ss.info["num_sweeps"] == SWEEPS
