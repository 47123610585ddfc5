"""bench.py's command line and its --dump-outputs writer (CPU only: no run of the benchmark itself)."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default_and_steps_are_validated():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _fake_step(R, n, seed=3):
    rng = np.random.RandomState(seed)
    states = rng.randint(0, 2, size=(R, n)).astype(np.uint8)
    energies = rng.normal(size=R)
    k = int(np.argmin(energies))
    best = (float(energies[k]), k, 0, states[k].copy())
    return best, states, energies, {"accepted": 12345, "proposals": 99999, "row_bytes": 0}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_step_in_float32_and_float64(tmp_path):
    best, states, energies, info = _fake_step(64, 100)
    bench.dump_outputs(str(tmp_path), best, states, energies, info)
    out = _load(str(tmp_path))
    assert sorted(out) == ["accepted_proposals", "best_energy", "best_replica_global_id", "best_state", "energies", "states"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["states"], states.astype(np.float32))
    assert np.array_equal(out["energies"], energies)
    assert out["best_energy"][0] == best[0] and out["best_replica_global_id"][0] == best[1]
    assert np.array_equal(out["best_state"], best[3].astype(np.float32))
    assert out["accepted_proposals"].tolist() == [12345.0, 99999.0]


def test_dump_outputs_samples_states_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200000)
    best, states, energies, info = _fake_step(512, 300)          # 614 KB of states as float32
    runs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        bench.dump_outputs(d, best, states, energies, info)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BYTES
        runs.append(_load(d))
    rows = runs[0]["states_replicas"].astype(np.int64)
    assert 0 < len(rows) < 512 and np.all(np.diff(rows) > 0)
    assert np.array_equal(runs[0]["states"], states[rows].astype(np.float32))
    assert np.array_equal(runs[0]["energies"], energies)                # the small arrays stay whole
    for name in runs[0]:                                                # the sample is fixed: same files, same values
        assert np.array_equal(runs[0][name], runs[1][name])
