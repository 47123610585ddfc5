"""``MI355XSampler`` -- the drop-in for the sampler objects the reference constructs in-line.

The reference solves its models by calling a dimod ``Sampler``:

    LeapHybridSampler().sample_qubo(Q, label=...)                       BQM_clustering.py:56-57
    FixedEmbeddingComposite(DWaveSampler(...), emb).sample_qubo(Q, label=, chain_strength=,
        num_reads=, return_embedding=True)                              BQM_clustering.py:67-75
    EmbeddingComposite(DWaveSampler()).sample_qubo(Q, ...)              BQM_clustering.py:84-85
    hybrid.KerberosSampler().sample(bqm, max_iter=, num_reads=, ...)    BQM_clustering.py:386
    LeapHybridDQMSampler().sample_dqm(dqm, label=...)                   DQM_clustering.py:45

``MI355XSampler`` offers the same four methods (plus ``sample_ising``) and returns a SampleSet
(sampleset.py).  QPU-only keyword arguments (``label``, ``chain_strength``, ``return_embedding``,
``time_limit``, Kerberos' ``max_iter/qpu_reads/tabu_timeout/qpu_params`` ...) are accepted and
ignored; the annealing arguments follow ``neal.SimulatedAnnealingSampler.sample`` (``num_reads``,
``num_sweeps``, ``beta_range``, ``beta_schedule_type``, ``beta_schedule``,
``num_sweeps_per_beta``, ``seed``, ``initial_states``, ``initial_states_generator``).

Everything numeric runs in the HIP library (libmi_sa.so); there is no CPU path.
"""
from __future__ import annotations

import os
import time
from typing import Any, Dict, Hashable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .bqm import BinaryQuadraticModel, DiscreteQuadraticModel
from .engine import Problem, energy_dense_f64, layout_block_for
from .models import (PottsModel, QuboModel, _csr_from_edges, default_beta_range,
                     make_beta_schedule, potts_energies_any, potts_merge_coefficients, potts_node_weight_groups,
                     potts_node_weights, qubo_dict_to_model)
from .metrics import cell_confidence, confidence_passes, connected_components, mean_pair_agreement, pac
from .sampleset import SampleSet, _unique_rows

# keyword arguments of the samplers the reference uses that have no meaning for an annealer on a GPU
_IGNORED_KWARGS = frozenset((
    "label", "chain_strength", "return_embedding", "time_limit", "annealing_time", "answer_mode",
    "auto_scale", "max_iter", "qpu_reads", "tabu_timeout", "qpu_params", "qpu_sampler",
    "convergence", "energy_threshold", "max_subproblem_size", "sa_reads", "sa_sweeps",
    "embedding_parameters", "chain_break_method", "chain_break_fraction", "warnings",
    "interrupt_function", "programming_thermalization", "readout_thermalization",
    "reduce_intersample_correlation", "num_spin_reversal_transforms", "flux_drift_compensation",
))

_DEFAULT_NUM_READS = 256


def _default_device() -> int:
    return int(os.environ.get("LOCAL_RANK", "0"))


class PendingSampleSet:
    """A sampler call whose anneal is enqueued on the GPU (``MI355XSampler.sample_qubo_async``); ``result()`` waits for it."""

    def __init__(self, steps):
        self._steps = steps
        self._value = None
        self._done = False
        self._advance()                                   # runs up to the enqueued anneal (or to the end: an empty model)

    def _advance(self):
        try:
            next(self._steps)
        except StopIteration as stop:
            self._value, self._done = stop.value, True

    def result(self) -> SampleSet:
        while not self._done:
            self._advance()
        return self._value

    def __del__(self):                                    # an abandoned call still releases its device buffers
        try:
            if not self._done:
                self._steps.close()
        except Exception:
            pass


class MI355XSampler:
    """Replica-parallel simulated annealing on one MI355X (one wavefront per replica)."""

    parameters = {
        "num_reads": [], "num_sweeps": [], "beta_range": [], "beta_schedule_type": [],
        "beta_schedule": [], "num_sweeps_per_beta": [], "seed": [], "initial_states": [],
        "initial_states_generator": [], "resync_interval": [], "kernel": [], "min_cluster_size": [],
        "merge_interval": [], "merge_proposals": [], "stability": [], "consensus": [], "split_disconnected": [],
        **{k: [] for k in _IGNORED_KWARGS},
    }
    properties = {"category": "software", "beta_schedule_options": ("linear", "geometric", "custom"),
                  "engine": "libmi_sa (HIP, gfx950)"}

    def __init__(self, device: Optional[int] = None, replica_offset: int = 0):
        self.device = _default_device() if device is None else int(device)
        self.replica_offset = int(replica_offset)
        _lib.load()                              # fail now, loudly, if the engine is not built

    # ------------------------------------------------------------------------------------------
    # public dimod-style surface
    # ------------------------------------------------------------------------------------------
    def sample_qubo(self, Q, **kwargs) -> SampleSet:
        """``Q``: dict ``{(u, v): bias}`` (BQM_clustering.py:36-47) or a ``models.QuboModel``."""
        offset = kwargs.pop("offset", 0.0)
        model = Q if isinstance(Q, QuboModel) else qubo_dict_to_model(Q, offset=offset)
        return self._sample_binary(model, "BINARY", kwargs)

    def sample_qubo_async(self, Q, **kwargs) -> "PendingSampleSet":
        """``sample_qubo`` in two halves: the model is uploaded and the anneal ENQUEUED on the problem's own stream when this
        returns; ``.result()`` waits for it and builds the SampleSet.  Independent calls overlap on the GPU -- what the
        two halves of a bisection are (clustering.py prefetches the second half while it descends into the first): with 500
        reads a call is one wavefront's latency on half of the chip's SIMDs."""
        offset = kwargs.pop("offset", 0.0)
        model = Q if isinstance(Q, QuboModel) else qubo_dict_to_model(Q, offset=offset)
        return PendingSampleSet(self._binary_steps(model, "BINARY", kwargs))

    def sample_ising(self, h, J, **kwargs) -> SampleSet:
        bqm = BinaryQuadraticModel.from_ising(h, J, kwargs.pop("offset", 0.0))
        return self.sample(bqm, **kwargs)

    def sample(self, bqm, **kwargs) -> SampleSet:
        """``bqm``: ``bqm.BinaryQuadraticModel``, a real ``dimod.BinaryQuadraticModel`` (duck-typed
        on ``linear`` / ``quadratic`` / ``offset`` / ``vartype``) or a ``models.QuboModel``."""
        if isinstance(bqm, QuboModel):
            return self._sample_binary(bqm, "BINARY", kwargs)
        vartype = getattr(bqm.vartype, "name", str(bqm.vartype))
        linear = dict(bqm.linear)
        quadratic = dict(bqm.quadratic)
        offset = float(bqm.offset)
        if vartype == "SPIN":
            # s = 2x - 1:  h s -> 2h x - h ;  J s_u s_v -> 4J x_u x_v - 2J x_u - 2J x_v + J
            Q: Dict[Tuple[Hashable, Hashable], float] = {}
            lin = {v: 2.0 * b for v, b in linear.items()}
            off = offset - sum(linear.values())
            for (u, v), b in quadratic.items():
                Q[(u, v)] = 4.0 * b
                lin[u] = lin.get(u, 0.0) - 2.0 * b
                lin[v] = lin.get(v, 0.0) - 2.0 * b
                off += b
            Qd = {(v, v): b for v, b in lin.items()}
            Qd.update(Q)
            model = qubo_dict_to_model(Qd, offset=off)
        elif vartype == "BINARY":
            Qd = {(v, v): b for v, b in linear.items()}
            Qd.update(quadratic)
            model = qubo_dict_to_model(Qd, offset=offset)
        else:
            raise ValueError("unsupported vartype %r" % (vartype,))
        return self._sample_binary(model, vartype, kwargs)

    def sample_dqm(self, dqm, **kwargs) -> SampleSet:
        """``dqm``: ``models.PottsModel``, ``bqm.DiscreteQuadraticModel`` or a real
        ``dimod.DiscreteQuadraticModel`` whose biases have the Potts shape `clustering_dqm` builds
        (DQM_clustering.py:29-43): case-independent linear biases, equal-case quadratic biases."""
        model = dqm if isinstance(dqm, PottsModel) else dqm_to_potts(dqm)
        return self._potts_run([model], self._split_kwargs(dict(kwargs)))[0]

    def sample_dqm_many(self, models, **kwargs) -> List[SampleSet]:
        """Several node-weighted Potts models that differ only in their pair coefficient and energy offset -- the
        modularity models of one graph at several resolutions (models.build_modularity_sweep) -- in ONE upload and ONE
        launch: model g runs as resolution group g (include/mi_sa.h mi_sa_problem_set_node_weight_groups), and its
        SampleSet equals ``sample_dqm(models[g], **kwargs)``.  ``num_reads`` is per model; ``num_sweeps``, ``seed``,
        ``initial_states`` (tiled to every group) and the sampler's ``replica_offset`` are shared.  The default schedule
        is each model's own (``default_potts_beta_range``); a ``beta_range`` of shape [2] or a ``beta_schedule`` applies
        to every model, one of shape [len(models), 2] gives each its own.  Every SampleSet's ``info`` has its own
        ``beta_range`` and a ``batch`` entry with what the groups share: the kernel time and name, the group count, the
        total proposals and accepted moves."""
        models = list(models)
        groups = potts_node_weight_groups(models)         # (refuses models that are not one graph's node-weighted ones)
        return self._potts_run(models, self._split_kwargs(dict(kwargs)), groups)

    # ------------------------------------------------------------------------------------------
    # internals
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _split_kwargs(kwargs: Dict[str, Any]):
        ignored = sorted(k for k in kwargs if k in _IGNORED_KWARGS)
        unknown = sorted(k for k in kwargs if k not in MI355XSampler.parameters)
        if unknown:
            raise TypeError("MI355XSampler got unexpected keyword argument(s): %s" % ", ".join(unknown))
        return {k: v for k, v in kwargs.items() if k not in _IGNORED_KWARGS}, ignored

    @staticmethod
    def _merge_kwargs(kw, min_size: int):
        """``merge_interval`` (0 / None = off) and ``merge_proposals`` (None = 2 K) of the Potts samplers, checked before
        any GPU work: merges empty clusters, so they do not combine with a minimum cluster size."""
        interval = kw.get("merge_interval")
        interval = 0 if interval is None else int(interval)
        proposals = kw.get("merge_proposals")
        if interval < 0:
            raise ValueError("'merge_interval' should be a non-negative integer")
        if proposals is not None and int(proposals) < 1:
            raise ValueError("'merge_proposals' should be a positive integer")
        if interval and (min_size or kw.get("min_cluster_size")):
            raise ValueError("merge moves together with min_cluster_size are not supported")
        return interval, (None if proposals is None else int(proposals))

    @staticmethod
    def _seed(seed) -> int:
        if seed is None:
            return int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31)
        if not isinstance(seed, (int, np.integer)) or seed < 0:
            raise TypeError("'seed' should be a non-negative integer")
        return int(seed)

    def _schedule(self, kw, range_fn):
        num_sweeps = int(kw.get("num_sweeps", 1000))
        if num_sweeps < 0:
            raise ValueError("'num_sweeps' should be a non-negative integer")
        stype = kw.get("beta_schedule_type", "geometric")
        beta_range = kw.get("beta_range")
        if stype != "custom" and beta_range is None:
            beta_range = range_fn()
        betas = make_beta_schedule(num_sweeps, beta_range if beta_range is not None else (1.0, 1.0),
                                   stype, int(kw.get("num_sweeps_per_beta", 1)),
                                   kw.get("beta_schedule"))
        if len(betas) and (np.any(betas <= 0) or not np.all(np.isfinite(betas))):
            raise ValueError("beta schedule must be positive and finite on this engine")
        return betas, (None if beta_range is None else [float(beta_range[0]), float(beta_range[1])]), stype

    @staticmethod
    def _initial_states(kw, variables, num_reads, vartype):
        """neal semantics: ``initial_states`` = (array, labels) / array / SampleSet; generator
        'none' | 'tile' | 'random'.  Returns (num_reads, array-or-None in BINARY/label form)."""
        init = kw.get("initial_states")
        gen = kw.get("initial_states_generator", "random")
        if gen not in ("none", "tile", "random"):
            raise ValueError("unknown value for 'initial_states_generator'")
        if init is None:
            if gen == "none":
                raise ValueError("initial_states_generator='none' requires initial_states")
            return (num_reads if num_reads is not None else _DEFAULT_NUM_READS), None
        labels = None
        if isinstance(init, SampleSet):
            arr, labels = init.record["sample"], init.variables
            if init.vartype == "SPIN" and vartype != "DISCRETE":
                arr = (arr + 1) // 2
        elif isinstance(init, tuple) and len(init) == 2:
            arr, labels = np.asarray(init[0]), list(init[1])
        elif isinstance(init, Mapping):
            labels = list(init.keys())
            arr = np.asarray([[init[v] for v in labels]])
        else:
            arr = np.asarray(init)
        if arr.ndim == 1:
            arr = arr[None, :]
        if labels is not None:
            pos = {v: i for i, v in enumerate(labels)}
            try:
                arr = arr[:, [pos[v] for v in variables]]
            except KeyError as exc:
                raise ValueError("initial_states is missing variable %r" % (exc.args[0],)) from exc
        if arr.shape[1] != len(variables):
            raise ValueError("initial_states has %d columns, model has %d variables"
                             % (arr.shape[1], len(variables)))
        if vartype == "SPIN" and not isinstance(init, SampleSet):
            if np.any((arr != 1) & (arr != -1)):
                raise ValueError("SPIN initial_states must be +-1")
            arr = (arr + 1) // 2
        if num_reads is None:
            num_reads = arr.shape[0]
        have = arr.shape[0]
        if have > num_reads:
            arr = arr[:num_reads]
        elif have < num_reads:
            if gen == "none":
                raise ValueError("insufficient initial states for num_reads with generator 'none'")
            if gen == "tile":
                reps = -(-num_reads // have)
                arr = np.tile(arr, (reps, 1))[:num_reads]
            else:                                 # 'random': remaining replicas start randomly --
                return num_reads, ("partial", arr)  # handled by the caller (device RNG rows)
        return num_reads, arr

    def _sample_binary(self, model: QuboModel, vartype: str, kwargs) -> SampleSet:
        return PendingSampleSet(self._binary_steps(model, vartype, kwargs)).result()

    def _binary_steps(self, model: QuboModel, vartype: str, kwargs):
        """Generator: everything up to the enqueued anneal, ONE ``yield``, then the fetch and the SampleSet (its return value)."""
        kw, ignored = self._split_kwargs(dict(kwargs))
        if kw.get("stability"):
            raise ValueError("'stability' (label agreement of the reads) applies to the Potts samplers (sample_dqm)")
        if kw.get("consensus"):
            raise ValueError("'consensus' (co-association of the reads) applies to the Potts samplers (sample_dqm)")
        if kw.get("split_disconnected"):
            raise ValueError("'split_disconnected' (connected components of the clusters) applies to the Potts samplers (sample_dqm)")
        t0 = time.perf_counter()
        n = model.num_variables
        if n == 0:
            return SampleSet(np.zeros((0, 0), dtype=np.int8), np.zeros(0), [], vartype,
                             info={"ignored_kwargs": ignored})
        seed = self._seed(kw.get("seed"))
        num_reads, init = self._initial_states(kw, model.variables, kw.get("num_reads"), vartype)
        if num_reads < 1:
            raise ValueError("'num_reads' should be a positive integer")
        betas, beta_range, stype = self._schedule(kw, lambda: default_beta_range(model))
        kernel = kw.get("kernel", "auto")
        if kernel not in ("auto", "dense", "csr"):
            raise ValueError("kernel must be 'auto', 'dense' or 'csr'")
        # structured models (sparse couplings + one uniform pair term: every graph-partition QUBO of the
        # reference) run on the CSR kernel at any size -- it is the faster one and needs no n x n matrix;
        # (rows wider than 64 neighbours on its runtime-width form); general QUBOs run on the dense kernels (n <= 65536)
        max_deg = int(np.diff(model.rowptr).max()) if n else 0
        use_csr = (kernel == "csr") or (kernel == "auto" and model._dense is None and (max_deg <= 4096 or n > 65536))
        if use_csr and model._dense is not None:
            raise ValueError("kernel='csr' needs a structured (CSR + uniform pair) model")
        if use_csr:
            prob = Problem.csr_rank1(model.rowptr, model.col, model.val.astype(np.float32),
                                     model.lin.astype(np.float32), float(np.float32(model.c_pair)),
                                     offset=model.offset, device=self.device, order="padded",
                                     energy_model=(model.val, model.lin, model.c_pair),
                                     block=layout_block_for(n, num_reads, max_deg), weights=model.weights)
        else:
            dense64 = model.dense_Qs()
            prob = Problem.dense(_symmetric_f32(dense64), offset=model.offset, device=self.device)
        with prob:
            init_arr = self._random_remainder(prob, num_reads, num_reads, seed, init[1]) if isinstance(init, tuple) else init
            t1 = time.perf_counter()
            prob.anneal(num_reads, betas, seed, self.replica_offset, init_arr,
                        int(kw.get("resync_interval", 0)))
            yield None                                # (enqueued: what follows waits for the run)
            states, dev_energy, stats = prob.fetch()
            kernel_ms = prob.kernel_ms()
            t2 = time.perf_counter()
        # energies in the caller's fp64 coefficients (what dimod's SampleSet.from_samples_bqm evaluates on the
        # host): the structured kernel evaluates them itself (energy_model above); the dense kernels report
        # the energies of the fp32 matrix they anneal, so that path runs the fp64 energy kernel on the samples
        energies = dev_energy if use_csr else energy_dense_f64(dense64, states, model.offset, self.device)
        samples = states.astype(np.int8)
        if vartype == "SPIN":
            samples = 2 * samples - 1
        info = self._info((betas, beta_range, stype), seed, num_reads, "csr_rank1" if use_csr else "dense", ignored,
                          self._launch_info(t0, t1, t2, kernel_ms, stats))
        info["device_energy_max_abs_diff"] = float(np.max(np.abs(dev_energy - energies)))
        if kwargs.get("return_embedding"):
            info["embedding_context"] = {"embedding": {}}    # read at BQM_clustering.py:79
        return SampleSet(samples, energies, model.variables, vartype, info=info)

    def _random_remainder(self, prob, replicas: int, num_reads: int, seed: int, have: np.ndarray) -> np.ndarray:
        """Initial states where fewer rows are given than there are reads ("partial", ``_initial_states``): the first
        ``num_reads`` rows of the device's own random initial states -- a zero-sweep anneal of all ``replicas``, fetched
        -- with the rows ``have`` written over the first of them."""
        prob.anneal(replicas, np.zeros(0), seed, self.replica_offset)
        rnd, _, _ = prob.fetch(energies=False)
        rnd = rnd[:num_reads]
        rnd[: have.shape[0]] = have
        return rnd

    @staticmethod
    def _launch_info(t0, t1, t2, kernel_ms, stats) -> Dict[str, Any]:
        """What one launch reports about itself in a sampleset's info: the wall-clock split, the kernel time, the moves."""
        return {"timing": {"upload_s": t1 - t0, "anneal_s": t2 - t1, "kernel_ms": kernel_ms},
                "updates_per_s": (stats["proposals"] / (kernel_ms * 1e-3)) if kernel_ms > 0 else None,
                "accepted": stats["accepted"], "proposals": stats["proposals"]}

    def _info(self, sched, seed, num_reads, kernel: str, ignored, launch: Dict[str, Any]) -> Dict[str, Any]:
        """The entries every sampleset's info has: the schedule ``sched`` (what ``_schedule`` returns), the run's
        arguments and ``launch`` -- ``_launch_info`` itself, or its ``batch`` form for the models of one launch."""
        betas, beta_range, stype = sched
        return {"beta_range": beta_range, "beta_schedule_type": stype, "seed": seed, "num_sweeps": int(len(betas)),
                "num_reads": int(num_reads), "kernel": kernel, "device": self.device, **launch,
                "energy_evaluation": "device fp64 (caller's coefficients)", "ignored_kwargs": ignored}

    def _potts_run(self, models: List[PottsModel], checked, groups=None) -> List[SampleSet]:
        """The one Potts run behind ``sample_dqm`` and ``sample_dqm_many``: ``models`` in ONE upload and ONE launch, one
        SampleSet each.  ``checked``: what ``_split_kwargs`` returns.  ``groups``: ``potts_node_weight_groups(models)``
        for the grouped entry, whose models run as resolution groups (a single one too) and report the launch under
        ``info["batch"]``; None for the single entry, which alone takes a model without node weights, a minimum cluster
        size and an empty model.  Every refusal comes before any GPU work."""
        kw, ignored = checked
        grouped = groups is not None
        wq, cw, w64, c64, offsets = groups if grouped else (None,) * 5
        G, m0 = len(models), models[0]
        n, K = m0.num_variables, m0.num_cases
        t0 = time.perf_counter()
        if n == 0:
            return [SampleSet(np.zeros((0, 0), dtype=np.int32), np.zeros(0), [], "DISCRETE",
                              info={"ignored_kwargs": ignored})]
        seed = self._seed(kw.get("seed"))
        num_reads, init = self._initial_states(kw, m0.variables, kw.get("num_reads"), "DISCRETE")
        if num_reads < 1:
            raise ValueError("'num_reads' should be a positive integer")
        ranges = kw.get("beta_range")
        per_model = grouped and ranges is not None and np.ndim(ranges) == 2
        if per_model and np.shape(ranges) != (G, 2):
            raise ValueError("a per-model beta_range needs shape [%d, 2]" % G)
        scheds = [self._schedule(dict(kw, beta_range=ranges[g]) if per_model else kw,
                                 lambda model=model: default_potts_beta_range(model)) for g, model in enumerate(models)]
        betas = np.stack([b for b, _, _ in scheds]) if grouped else scheds[0][0]
        _check_consensus(kw, K, num_reads)
        # the CQM's "every cluster has at least m members" (CQM_clustering.py:46-48): a hard constraint on moves
        min_size = int(kw.get("min_cluster_size", 0 if grouped else m0.info.get("min_cluster_size", 0)) or 0)
        _check_split(kw, min_size, models)
        if m0.node_weight is not None and min_size > 0:
            raise ValueError("node weights (a modularity model) together with min_cluster_size are not supported")
        merge_interval, merge_proposals = self._merge_kwargs(kw, min_size)
        if min_size * K > n:
            raise ValueError("min_cluster_size %d x %d clusters exceeds the %d variables" % (min_size, K, n))
        prob = Problem.potts_csr(m0.rowptr, m0.col, m0.val.astype(np.float32), float(np.float32(m0.c_pair)), n, K,
                                 lin_offset=m0.lin_offset, device=self.device, order="padded",
                                 energy_model=(m0.val, m0.c_pair),
                                 node_weights=(wq, cw[0], w64) if grouped else potts_node_weights(m0))
        with prob:
            if grouped:
                prob.set_node_weight_groups(cw, c64, offsets)
            if merge_interval:
                prob.set_merge_moves(merge_interval, merge_proposals, potts_merge_coefficients(models))
            init_arr = init
            if isinstance(init, tuple) or (min_size > 0 and init is None):    # (every group starts from group 0's rows)
                have = init[1] if isinstance(init, tuple) else np.zeros((0, n), dtype=np.uint16)
                init_arr = self._random_remainder(prob, num_reads * G, num_reads, seed, have)
            if min_size > 0:
                init_arr = _make_feasible(np.array(init_arr, dtype=np.uint16, copy=True), K, min_size)
                prob.set_option("min_cluster_size", min_size)
            if grouped and init_arr is not None:
                init_arr = np.tile(np.asarray(init_arr, dtype=np.uint16), (G, 1))
            t1 = time.perf_counter()
            prob.anneal(num_reads * G, betas, seed, self.replica_offset, init_arr)
            labels, energies, stats = prob.fetch()       # (energies: on the device, in the models' fp64 coefficients)
            kernel_ms = prob.kernel_ms()
            kernel_name = prob.kernel_name() if grouped else None
            merges = prob.merges_accepted() if merge_interval else None
            agree = prob.label_agreement(G) if kw.get("stability") and num_reads >= 2 else None
            cons = _consensus_info(prob, G, m0, num_reads) if kw.get("consensus") else None
            comps = prob.components()[0] if kw.get("split_disconnected") else None    # (all groups in one call)
            t2 = time.perf_counter()
        launch = self._launch_info(t0, t1, t2, kernel_ms, stats)
        if grouped:                                       # what the groups share, as ONE object: the launch was one
            del launch["timing"]["kernel_ms"]
            launch = {"batch": {"groups": G, "kernel_ms": kernel_ms, "kernel_name": kernel_name, **launch}}
        out = []
        for g, model in enumerate(models):
            rows = slice(g * num_reads, (g + 1) * num_reads)
            info = self._info(scheds[g], seed, num_reads, "potts_csr", ignored, launch)
            if merge_interval:
                info["merges_accepted"] = merges                  # (all groups together, like "batch")
            if kw.get("stability"):
                info["stability"], info["stability_nmi"] = (
                    mean_pair_agreement(agree["ari"][g], agree["nmi"][g]) if agree is not None else (None, None))
            if cons is not None:
                info.update(cons[g])
            if comps is not None:
                info.update(_split_info(model, labels[rows], energies[rows], comps[rows]))
            out.append(SampleSet(labels[rows].astype(np.int32), energies[rows], model.variables, "DISCRETE", info=info))
        return out


MAX_CONSENSUS_READS = 8192                 # MI_COASSOC_MAX_READS (include/mi_metrics.h)


def model_edges(model):
    """The model's edges as (eu, ev) index arrays into ``model.variables``: every stored pair once, eu < ev, sorted."""
    n = model.num_variables
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(model.rowptr, dtype=np.int64)))
    cols = np.asarray(model.col, dtype=np.int64)
    keep = rows != cols
    lo, hi = np.minimum(rows[keep], cols[keep]), np.maximum(rows[keep], cols[keep])
    key = np.unique(lo * n + hi)
    return (key // n).astype(np.int32), (key % n).astype(np.int32)


def _consensus_info(prob, G: int, model, num_reads: int):
    """Per resolution group the ``consensus=True`` entries of a sampleset's info, from the states in HBM: the model's own
    edges, the share of reads that keep each inside a cluster, PAC, the components of the edges kept by at least half
    of the reads, and every cell's confidence in its component."""
    eu, ev = model_edges(model)
    n = model.num_variables
    first = prob.coassociation(G, edges=(eu, ev))
    hist = first["hist"].reshape(G, -1)
    edge = first["edge_counts"].reshape(G, -1)
    # the components of the edges kept by at least half of the reads, every group in one launch (what
    # metrics.consensus_labels restates on the host)
    labs = connected_components((eu, ev), n, keep=edge >= 0.5 * num_reads, device=prob.device)[0].astype(np.int64)
    # confidence: one dense pass per 63 non-singleton components, the references of ALL groups in the same call
    passes = [confidence_passes(labs[g]) for g in range(G)]
    conf = [np.ones(n) for _ in range(G)]
    for k in range(max(len(ps) for ps in passes)):
        refs = np.zeros((G, n), dtype=np.int64)
        for g in range(G):
            if k < len(passes[g]):
                refs[g] = passes[g][k][0]
        rs = prob.coassociation(G, ref=refs, hist=False)["rowsum"].reshape(G, n, -1)
        for g in range(G):
            if k < len(passes[g]):
                ref, inside = passes[g][k]
                conf[g][inside] = cell_confidence(rs[g], ref, num_reads)[inside]
    return [{"pac": pac(hist[g]), "edge_cooccurrence": edge[g].astype(np.float64) / float(num_reads),
             "consensus_edges": (eu, ev), "consensus_labels": labs[g], "cell_confidence": conf[g]} for g in range(G)]


def _check_split(kw, min_size: int, models):
    """``split_disconnected=True`` is refused before any GPU work where the split could break a constraint or raise the
    energy: with a minimum cluster size, and with a negative pair coefficient (the pair terms a split removes must be
    >= 0 for the refined labelling to be no worse)."""
    if not kw.get("split_disconnected"):
        return
    if min_size > 0:
        raise ValueError("'split_disconnected' together with min_cluster_size is not supported: a split can leave a "
                         "cluster below the minimum size")
    for m in models:
        if m.c_pair < 0.0:
            raise ValueError("'split_disconnected' needs a non-negative pair coefficient (got %r): the split of a "
                             "disconnected cluster could raise the energy" % (m.c_pair,))


def _split_info(model, labels, energies, comps):
    """The ``split_disconnected=True`` entries of a sampleset's info: the reads' refined labellings ``comps`` brought into
    record order (SampleSet keeps the first read of every distinct sample, sorted by energy, stable), their cluster
    counts and their energies in the model's fp64 coefficients."""
    labels, energies = np.asarray(labels), np.asarray(energies, dtype=np.float64)
    first = _unique_rows(labels)[1] if len(energies) > 1 else np.arange(len(energies))
    first = np.asarray(first)[np.argsort(energies[first], kind="stable")]
    split = np.ascontiguousarray(comps[first], dtype=np.int32)
    return {"split_labels": split, "split_num_clusters": (split.max(axis=1) + 1).astype(np.int64),
            "split_energy": potts_energies_any(model, split)}


def _check_consensus(kw, num_cases: int, num_reads: int):
    """``consensus=True`` is refused before any GPU work where the co-association pass could not run after the anneal."""
    if not kw.get("consensus"):
        return
    if num_cases > 64:
        raise ValueError("'consensus' needs at most 64 cases per variable (got %d)" % num_cases)
    if num_reads > MAX_CONSENSUS_READS:
        raise ValueError("'consensus' needs at most %d reads per model (got %d)" % (MAX_CONSENSUS_READS, num_reads))


def _make_feasible(labels: np.ndarray, K: int, min_size: int) -> np.ndarray:
    """Deterministic repair of initial labelings that leave a cluster below ``min_size``: members of the
    largest clusters (highest indices first) are moved into the deficient ones."""
    for r in range(labels.shape[0]):
        cnt = np.bincount(labels[r], minlength=K)
        for c in np.where(cnt < min_size)[0]:
            while cnt[c] < min_size:
                big = int(np.argmax(cnt))
                i = int(np.where(labels[r] == big)[0][-1])
                labels[r, i] = c
                cnt[big] -= 1
                cnt[c] += 1
    return labels


def _symmetric_f32(Qs64: np.ndarray) -> np.ndarray:
    """fp64 symmetric -> fp32 symmetric (rounding each entry once keeps symmetry)."""
    Q = np.asarray(Qs64, dtype=np.float64).astype(np.float32)
    return np.ascontiguousarray(Q)


def default_potts_beta_range(model: PottsModel) -> Tuple[float, float]:
    """Hot: the largest possible single-move |dE| gets acceptance 1/2; cold: the smallest non-zero
    coupling gets acceptance 1/100 (the neal rule applied to the move set of the Potts chain)."""
    n = model.num_variables
    rows = np.repeat(np.arange(n), np.diff(model.rowptr))
    if model.node_weight is not None:
        # node weights: the pair u, v of one cluster carries c w_u w_v (w_u w_v on the stored pairs as well)
        w = np.asarray(model.node_weight, dtype=np.float64)
        cww = abs(model.c_pair) * w[rows] * w[model.col]
        full = model.val + model.c_pair * w[rows] * w[model.col]
        abs_sum = np.zeros(n)
        np.add.at(abs_sum, rows, np.abs(full) - cww)
        abs_sum += abs(model.c_pair) * w * (float(np.sum(w)) - w)
        max_field = float(abs_sum.max()) if n else 1.0
        cands = np.abs(full[full != 0.0])
        min_bias = float(cands.min()) if len(cands) else 1.0
        if max_field <= 0:
            max_field = 1.0
        return float(np.log(2.0) / max_field), float(np.log(100.0) / min_bias)
    full = model.val + model.c_pair
    abs_sum = np.zeros(n)
    np.add.at(abs_sum, rows, np.abs(full) - abs(model.c_pair))
    abs_sum += abs(model.c_pair) * (n - 1)
    max_field = float(abs_sum.max()) if n else 1.0
    cands = np.abs(full[full != 0.0])
    if model.c_pair != 0.0:
        cands = np.concatenate([cands, [abs(model.c_pair)]])
    min_bias = float(cands.min()) if len(cands) else 1.0
    if max_field <= 0:
        max_field = 1.0
    return float(np.log(2.0) / max_field), float(np.log(100.0) / min_bias)


def dqm_to_potts(dqm) -> PottsModel:
    """Reduce a (look-alike or real dimod) DiscreteQuadraticModel to Potts form, verifying that it
    has the shape `clustering_dqm` builds.  Raises NotImplementedError otherwise."""
    variables = list(dqm.variables)
    n = len(variables)
    if n == 0:
        return PottsModel([], 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0.0,
                          np.zeros(0))
    K = int(dqm.num_cases(variables[0]))
    index = {v: i for i, v in enumerate(variables)}
    lin = np.zeros(n)
    for v in variables:
        if int(dqm.num_cases(v)) != K:
            raise NotImplementedError("all variables must have the same number of cases")
        b = np.asarray(dqm.get_linear(v), dtype=np.float64)
        if np.any(b != b[0]):
            raise NotImplementedError("case-dependent linear biases are not in Potts form")
        lin[index[v]] = b[0]
    if isinstance(dqm, DiscreteQuadraticModel):
        pairs = [(u, v, tab) for (u, v), tab in dqm.interactions()]
    else:                                         # real dimod DQM
        pairs = []
        for u in variables:
            for v in dqm.adj[u]:
                if index[u] < index[v]:
                    pairs.append((u, v, dqm.get_quadratic(u, v)))
    eu = np.empty(len(pairs), dtype=np.int32)
    ev = np.empty(len(pairs), dtype=np.int32)
    b = np.empty(len(pairs), dtype=np.float64)
    for k, (u, v, tab) in enumerate(pairs):
        vals = set()
        for (cu, cv), x in tab.items():
            if cu != cv:
                if x != 0.0:
                    raise NotImplementedError("unequal-case quadratic biases are not in Potts form")
            else:
                vals.add(x)
        if len(vals) > 1 or (vals and len([1 for (cu, cv) in tab if cu == cv]) != K):
            raise NotImplementedError("case-dependent quadratic biases are not in Potts form")
        eu[k], ev[k] = index[u], index[v]
        b[k] = vals.pop() if vals else 0.0
    c_pair = 0.0
    npairs = n * (n - 1) // 2
    if len(b) and 2 * len(b) >= npairs:
        vals_u, counts = np.unique(b, return_counts=True)
        top = int(np.argmax(counts))
        if 2 * counts[top] >= npairs:
            c_pair = float(vals_u[top])
    if c_pair != 0.0:
        dense = np.zeros((n, n))
        lo, hi = np.minimum(eu, ev), np.maximum(eu, ev)
        dense[lo, hi] = b
        iu, ju = np.triu_indices(n, 1)
        resid = dense[iu, ju] - c_pair
        nz = resid != 0.0
        rowptr, col, val = _csr_from_edges(n, iu[nz].astype(np.int32), ju[nz].astype(np.int32),
                                           resid[nz])
    else:
        rowptr, col, val = _csr_from_edges(n, eu, ev, b)
    return PottsModel(variables, K, rowptr, col, val, c_pair, lin, info={"kind": "dqm"})
