"""Thin object layer over the C ABI: one ``Problem`` = one model resident in HBM on one GPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib


_POTTS_MAX_N = 40000          # mi_sa_problem_create_potts_csr_f32's limit


def layout_block_for(n: int, num_reads: int, max_degree: int = 16):
    """Seats per edge-free block the sampler lays a structured binary model out in: 64 (one wavefront sweeps a slot per
    step), or ``"auto"`` for the few reads the reference asks for (``num_reads = 500``, BQM_clustering.py:52), where
    every wavefront has a SIMD to itself and a run takes (steps per sweep) x (one wavefront's time per step):
    ``Problem.csr_rank1`` then plans the 64-seat AND the 128-seat layout and takes the wider one when it needs few
    enough blocks -- one wavefront sweeps such a block per step (K2w, csrc/sparse_split_kernels.hip: with the thresholds
    coming from the workgroup's second wavefront a two-slot step takes 1.86 times a one-slot step) -- which large sparse
    graphs do (n = 2638: 22 blocks against 42 slots) and small or clustered ones, whose block count is set by the
    colours they need, do not."""
    if num_reads > 1024 or max_degree > 32 or n > 16384 or n < 1024:     # (below ~1000 variables the colours decide)
        return 64
    return "auto"


# a two-slot step of the wide kernel against a one-slot step (MI355X, a wavefront alone on its SIMD, thresholds from the
# second wavefront of its workgroup, field sums staged behind counted LDS waits: 439 ns per 128-seat block, 236 ns per
# 64-seat slot at n = 2638, 500 reads)
_WIDE_STEP_RATIO = 439.0 / 236.0


class Problem(_lib.Handle):
    """A model uploaded to one MI355X.  ``anneal`` is asynchronous; ``fetch``/``best`` wait."""
    _destroy = "mi_sa_problem_destroy"

    def __init__(self, handle, kind, n, num_cases, device, perm=None, seats=None, n_dev=None):
        self._h = handle
        self.kind = kind
        self.n = n                       # variables of the CALLER's model
        self.num_cases = num_cases
        self.device = device
        self._last = None
        self.perm = perm                 # device variable j is the caller's variable perm[j] (None: identity / padded)
        # device column of the caller's variable i (None: identity), and the device-side variable count: larger than
        # n under order="padded", where the seats no variable sits in are holes that stay 0
        self._inv = None if perm is None else np.argsort(perm)
        if seats is not None:
            self._inv = np.asarray(seats, dtype=np.int64)
        self.n_dev = int(n if n_dev is None else n_dev)
        self.groups = 1                  # resolution groups (set_node_weight_groups)

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def dense(cls, Qs: np.ndarray, offset: float = 0.0, device: int = 0) -> "Problem":
        """``E(x) = x^T Qs x + offset`` with Qs symmetric (diag = linear terms)."""
        Qs = np.ascontiguousarray(Qs, dtype=np.float32)
        if Qs.ndim != 2 or Qs.shape[0] != Qs.shape[1]:
            raise ValueError("Qs must be a square matrix")
        if not np.array_equal(Qs, Qs.T):
            raise ValueError("Qs must be symmetric (use (Q + Q.T)/2 with the diagonal kept)")
        h = C.c_void_p()
        _lib.call("mi_sa_problem_create_dense_f32", Qs, Qs.shape[0], float(offset), int(device), h)
        return cls(h, _lib.KIND_DENSE, Qs.shape[0], 2, device)

    @classmethod
    def csr_rank1(cls, rowptr, col, val, lin, c_pair: float, offset: float = 0.0,
                  device: int = 0, order: Optional[str] = None, energy_model=None, block=64, weights=None) -> "Problem":
        """``order="slots"`` renumbers the variables on the device so that the 64 variables a wavefront
        sweeps together are (as far as possible) mutually non-adjacent -- the kernel's integer fast path
        (models.slot_independent_order).  States go in and come out in the CALLER's order either way; the
        chain is a different (equally valid) sweep order, so results differ from ``order=None`` runs.
        ``order="padded"``: the same with holes allowed -- as many blocks of 64 seats as it takes to keep EVERY edge
        between blocks (models.padded_slot_layout); what small or strongly clustered graphs need (the subgraphs of the
        reference's recursive bisection, its 256-node benchmark graphs), where no packed order is edge-free.

        ``block`` (64, 128, 256 or "auto"; ``order="padded"`` only): seats per edge-free block.  128 / 256 lay the model
        out for the few-replica kernels (csrc/sparse_split_kernels.hip: one wavefront sweeps a whole block per step, K2w,
        or -- option ``k2_wide`` = 2 -- a workgroup of 2 / 4 wavefronts does, K2s), which the library picks for runs of up
        to 1024 replicas; "auto" plans both the 64- and the 128-seat layout and keeps the faster; ``layout_block_for`` is
        the sampler's choice.

        ``energy_model=(val64, lin64, c_pair64)``: the caller's fp64 coefficients (same CSR structure); the
        reported energies are then evaluated on the device in that model (the chain itself runs in fp32).

        ``weights`` (positive integers, ``order="padded"`` only): weights of the pair term, ``c_pair a_i a_j`` on pair
        (i, j) -- the slack bits of a squared linear constraint (models.add_size_window_penalty).  The variables whose
        weight is not 1 (at most 64, without sparse couplings) get a 64-seat slot of their own behind the others."""
        if weights is not None:
            weights = np.asarray(weights, dtype=np.int64)
            if np.all(weights == 1):
                weights = None
        if weights is not None:
            return cls._csr_rank1_weighted(rowptr, col, val, lin, c_pair, offset, device, order, energy_model, weights)
        perm = None
        val64 = lin64 = None
        if energy_model is not None:
            val64, lin64 = np.asarray(energy_model[0], dtype=np.float64), np.asarray(energy_model[1], dtype=np.float64)
        if order == "slots":
            from .models import permute_csr, slot_independent_order
            perm = slot_independent_order(rowptr, col)
            if val64 is not None:
                rowptr, col, val, val64 = permute_csr(rowptr, col, val, perm, also=val64)
                lin64 = lin64[perm]
            else:
                rowptr, col, val = permute_csr(rowptr, col, val, perm)
            lin = np.asarray(lin)[perm]
        elif order == "padded":
            # seats with holes (models.padded_slot_layout): the fewest blocks of 64 that keep every edge BETWEEN blocks.
            # A hole is a variable without couplings whose linear term is +inf: the kernels start it at 0 and
            # never flip it; its fp64 energy coefficients are 0.
            from .models import pad_csr, padded_slot_layout
            if block == "auto":
                # both layouts planned (a millisecond each); the 128-seat one when its steps take less time in all
                s64 = padded_slot_layout(rowptr, col, slot=64)
                s128 = padded_slot_layout(rowptr, col, slot=128)
                wide = s128[2] == 0 and s64[2] == 0 and (s128[1] + (s128[1] & 1)) * _WIDE_STEP_RATIO < s64[1]
                block = 128 if wide else 64
                seats, nslots, clashes = s128 if wide else s64
            elif block in (64, 128, 256):
                seats, nslots, clashes = padded_slot_layout(rowptr, col, slot=block)
            else:
                raise ValueError("block must be 64, 128, 256 or 'auto'")
            if block > 64 and clashes:               # no edge-free layout in blocks this wide: the 64-seat layout
                return cls.csr_rank1(rowptr, col, val, lin, c_pair, offset, device, "padded", energy_model)
            # rows wider than 64 neighbours (untrimmed SNN graphs) run on the runtime-width kernel, whose cost per slot is
            # the adjacency it streams whether a seat holds a variable or not: a layout that needs many more slots than the
            # packed one costs more than the serial accept loop it avoids (degree 110: 82 slots against 42, 1.4e10
            # against 2.6e10 updates/s) -- the packed slot-independent order there
            if int(np.diff(np.asarray(rowptr)).max(initial=0)) > 64 and nslots * block * 5 > ((len(lin) + 63) // 64) * 64 * 6:
                return cls.csr_rank1(rowptr, col, val, lin, c_pair, offset, device, "slots", energy_model)
            if block == 128 and nslots % 2:          # (the two-wavefront kernel takes whole groups of four 64-seat slots)
                nslots += 1
            n_caller, n_dev = len(lin), nslots * block
            if n_dev > (1 << 20) >= n_caller:        # the holes would push the model over the kernel's size limit
                return cls.csr_rank1(rowptr, col, val, lin, c_pair, offset, device, "slots", energy_model)
            if val64 is not None:
                rowptr, col, val, val64 = pad_csr(rowptr, col, val, seats, n_dev, also=val64)     # (one sort for both)
                l64 = np.zeros(n_dev, dtype=np.float64)
                l64[seats] = lin64
                lin64 = l64
            else:
                rowptr, col, val = pad_csr(rowptr, col, val, seats, n_dev)
            lpad = np.full(n_dev, np.inf, dtype=np.float32)
            lpad[seats] = np.asarray(lin, dtype=np.float32)
            lin = lpad
        elif order is not None:
            raise ValueError("order must be None, 'slots' or 'padded'")
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        lin = np.ascontiguousarray(lin, dtype=np.float32)
        n = len(lin)
        h = C.c_void_p()
        _lib.call("mi_sa_problem_create_csr_rank1_f32", rowptr, col, val, lin, float(c_pair), n, float(offset), int(device), h)
        if order == "padded":
            prob = cls(h, _lib.KIND_CSR_RANK1, n_caller, 2, device, seats=seats, n_dev=n_dev)
        else:
            prob = cls(h, _lib.KIND_CSR_RANK1, n, 2, device, perm=perm)
        if val64 is not None:
            prob._set_energy_model(val64, lin64, float(energy_model[2]), len(val))
        return prob

    @classmethod
    def _csr_rank1_weighted(cls, rowptr, col, val, lin, c_pair, offset, device, order, energy_model, weights) -> "Problem":
        """A model with pair-term weights in its padded layout (``weighted_layout_csr``);
        mi_sa_problem_set_pair_weights."""
        if order != "padded":
            raise ValueError("a model with pair-term weights needs order='padded'")
        n_caller = len(lin)
        rp, cc, vv, lpad, wdev, seats, n_dev, val64, lin64 = weighted_layout_csr(rowptr, col, val, lin, weights, energy_model)
        h = C.c_void_p()
        _lib.call("mi_sa_problem_create_csr_rank1_f32", rp, cc, vv, lpad, float(c_pair), n_dev, float(offset), int(device), h)
        prob = cls(h, _lib.KIND_CSR_RANK1, n_caller, 2, device, seats=seats, n_dev=n_dev)
        try:
            _lib.call("mi_sa_problem_set_pair_weights", h, wdev)
        except Exception:
            prob.close()
            raise
        if val64 is not None:
            prob._set_energy_model(val64, lin64, float(energy_model[2]), len(vv))
        return prob

    @classmethod
    def potts_csr(cls, rowptr, col, val, c_pair: float, n: int, num_cases: int,
                  lin_offset: float = 0.0, device: int = 0, order: Optional[str] = None,
                  energy_model=None, node_weights=None) -> "Problem":
        """``order="slots"`` / ``"padded"``: as in :meth:`csr_rank1` (labels go in and come out in the caller's order).
        ``energy_model=(val64, c_pair64)``: fp64 coefficients for the reported energies.
        ``node_weights=(wq, cw, w64)``: node weights of the pair term in the caller's order (:meth:`set_node_weights`)."""
        perm = None
        val64 = None if energy_model is None else np.asarray(energy_model[0], dtype=np.float64)
        if order == "slots":
            from .models import permute_csr, slot_independent_order
            perm = slot_independent_order(rowptr, col)
            if val64 is not None:
                rowptr, col, val, val64 = permute_csr(rowptr, col, val, perm, also=val64)
            else:
                rowptr, col, val = permute_csr(rowptr, col, val, perm)
        elif order == "padded":
            # seats with holes, as in csr_rank1; a hole of a Potts model is marked through mi_sa_problem_set_absent:
            # label 0, in no cluster, never proposed
            from .models import pad_csr, padded_slot_layout
            seats, nslots, _ = padded_slot_layout(rowptr, col)
            if nslots * 64 > _POTTS_MAX_N >= int(n):  # the holes would push the model over the kernel's size limit (its
                # LDS budget is checked against the padded size): the packed order, clashing slots on the general path
                return cls.potts_csr(rowptr, col, val, c_pair, n, num_cases, lin_offset, device, "slots", energy_model,
                                     node_weights)
            n_caller, n = int(n), nslots * 64
            if val64 is not None:
                rowptr, col, val, val64 = pad_csr(rowptr, col, val, seats, n, also=val64)
            else:
                rowptr, col, val = pad_csr(rowptr, col, val, seats, n)
        elif order is not None:
            raise ValueError("order must be None, 'slots' or 'padded'")
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        h = C.c_void_p()
        _lib.call("mi_sa_problem_create_potts_csr_f32", rowptr, col, val, float(c_pair), int(n), int(num_cases),
                  float(lin_offset), int(device), h)
        if order == "padded":
            prob = cls(h, _lib.KIND_POTTS_CSR, n_caller, int(num_cases), device, seats=seats, n_dev=n)
            absent = np.ones(n, dtype=np.uint8)
            absent[seats] = 0
            try:
                _lib.call("mi_sa_problem_set_absent", h, absent)
            except Exception:
                prob.close()
                raise
        else:
            prob = cls(h, _lib.KIND_POTTS_CSR, int(n), int(num_cases), device, perm=perm)
        if val64 is not None:
            prob._set_energy_model(val64, None, float(energy_model[1]), len(val))
        if node_weights is not None:
            try:
                prob.set_node_weights(*node_weights)
            except Exception:
                prob.close()
                raise
        return prob

    def set_node_weights(self, wq, cw, w64=None):
        """Potts problems: integer node weights ``wq`` (>= 0, sum <= 2^30) of the pair term, their fp32 coefficients
        ``cw`` and fp64 weights ``w64`` for the reported energies (default ``wq``), in the caller's variable order
        (chain 2d, include/mi_sa.h mi_sa_problem_set_node_weights).  Holes of a padded layout get weight 0.  Call
        before the first anneal."""
        wq = np.asarray(wq)
        cw = np.asarray(cw, dtype=np.float32)
        w64 = None if w64 is None else np.asarray(w64, dtype=np.float64)
        if wq.shape != (self.n,) or cw.shape != (self.n,) or (w64 is not None and w64.shape != (self.n,)):
            raise ValueError("node weights need one entry per variable (%d)" % self.n)
        if np.any(wq < 0) or np.any(wq > np.iinfo(np.int32).max):
            raise ValueError("node weights must be non-negative int32 values")
        cols = np.arange(self.n) if self._inv is None else self._inv
        dq = np.zeros(self.n_dev, dtype=np.int32)
        dc = np.zeros(self.n_dev, dtype=np.float32)
        dw = np.zeros(self.n_dev, dtype=np.float64)
        dq[cols] = wq.astype(np.int32)
        dc[cols] = cw
        dw[cols] = wq.astype(np.float64) if w64 is None else w64
        _lib.call("mi_sa_problem_set_node_weights", self._handle(), dq, dc, dw)

    def set_node_weight_groups(self, cw, c64, offset):
        """Resolution groups of a problem with node weights (include/mi_sa.h mi_sa_problem_set_node_weight_groups):
        ``cw`` [G, n] fp32 coefficients in the caller's variable order, ``c64`` / ``offset`` [G] the fp64 pair coefficient
        and energy offset of each group.  An anneal of R replicas then runs G groups of R / G consecutive replicas, each
        keyed by its index inside the group (group g = the single-resolution run of its own tables, same seed); ``betas``
        of shape [G, num_sweeps] give each group its own schedule.  Holes of a padded layout get 0.  Call after
        :meth:`set_node_weights` and before the first anneal."""
        cw = np.asarray(cw, dtype=np.float32)
        c64 = np.ascontiguousarray(c64, dtype=np.float64)
        offset = np.ascontiguousarray(offset, dtype=np.float64)
        if cw.ndim != 2 or cw.shape[1] != self.n:
            raise ValueError("cw must have shape [G, n] with n = %d" % self.n)
        G = cw.shape[0]
        if c64.shape != (G,) or offset.shape != (G,):
            raise ValueError("c64 and offset need one entry per group (%d)" % G)
        cols = np.arange(self.n) if self._inv is None else self._inv
        dc = np.zeros((G, self.n_dev), dtype=np.float32)
        dc[:, cols] = cw
        _lib.call("mi_sa_problem_set_node_weight_groups", self._handle(), int(G), dc, c64, offset)
        self.groups = int(G)

    def set_merge_moves(self, interval: int, proposals: Optional[int] = None, cq=None):
        """Potts problems: merge moves (chain 2e, include/mi_sa.h mi_sa_problem_set_merge_moves).  Every anneal then runs
        a merge phase of ``proposals`` proposals (default ``2 K``) before each global sweep ``s > 0`` with
        ``s % interval == 0``; ``interval = 0`` turns merges off.  ``cq``: the coefficient of the cluster-sum product per
        resolution group (``models.potts_merge_coefficients``; required with node weights), None = ``c_pair``.  Call
        after :meth:`set_node_weight_groups`."""
        if proposals is None:
            proposals = 2 * int(self.num_cases)
        cq_arr = None
        if cq is not None:
            cq_arr = np.ascontiguousarray(np.atleast_1d(np.asarray(cq, dtype=np.float64)))
            if cq_arr.shape != (self.groups,):
                raise ValueError("cq needs one value per resolution group (%d)" % self.groups)
        _lib.call("mi_sa_problem_set_merge_moves", self._handle(), int(interval), int(proposals), cq_arr)

    def merges_accepted(self) -> int:
        """Merges the merge phases of the last anneal accepted (mi_sa_debug_stats word 4)."""
        return int(self.debug_stats(5)[4])

    def _set_energy_model(self, val64, lin64, c_pair64, nnz):
        if len(val64) != nnz or (lin64 is not None and len(lin64) != self.n_dev):
            self.close()
            raise ValueError("energy_model must have the structure of the fp32 model")
        val64 = np.ascontiguousarray(val64, dtype=np.float64)
        lin64 = None if lin64 is None else np.ascontiguousarray(lin64, dtype=np.float64)
        try:
            _lib.call("mi_sa_problem_set_energy_model_f64", self._handle(), val64, lin64, float(c_pair64))
        except Exception:
            self.close()
            raise

    def set_option(self, key: str, value: int):
        _lib.call("mi_sa_set_option", self._handle(), key.encode(), int(value))

    def debug_pace(self, words: int = 288):
        out = np.zeros(words, dtype=np.uint32)
        _lib.call("mi_sa_debug_pace", self._handle(), out, words)
        return out

    def debug_stats(self, words: int = 16):
        out = np.zeros(words, dtype=np.uint64)
        _lib.call("mi_sa_debug_stats", self._handle(), out, words)
        return out

    # -- the anneal -----------------------------------------------------------------------------
    @property
    def state_dtype(self):
        return np.uint16 if self.kind == _lib.KIND_POTTS_CSR else np.uint8

    def anneal(self, num_reads: int, betas, seed: int, replica_offset: int = 0,
               initial_states: Optional[np.ndarray] = None, resync_interval: int = 0,
               sweep_offset: int = 0, continue_run: bool = False, num_sweeps: Optional[int] = None):
        """``betas``: one per sweep (default), or -- when ``num_sweeps`` is given -- one per REPLICA, held
        constant for ``num_sweeps`` sweeps (a tempering rung); ``betas=None`` with ``num_sweeps``: every replica
        at the temperature the device-side tempering state holds for it (``tempering_begin`` / ``_exchange``).
        ``continue_run`` starts from the states the previous call left on the device; ``sweep_offset`` continues
        its random stream.  With resolution groups (:meth:`set_node_weight_groups`) ``betas`` may have shape
        [G, num_sweeps]: one schedule per group (else every group uses the one given)."""
        resident = betas is None
        if resident and num_sweeps is None:
            raise ValueError("betas=None (temperatures resident on the device) needs num_sweeps")
        betas = None if resident else np.ascontiguousarray(betas, dtype=np.float64)
        per_replica = num_sweeps is not None
        per_group = not resident and betas.ndim == 2
        if per_group and (per_replica or betas.shape[0] != self.groups):
            raise ValueError("per-group betas need shape [G, num_sweeps] with G = %d groups" % self.groups)
        if per_replica and not resident and len(betas) != num_reads:
            raise ValueError("per-replica betas need one entry per replica")
        flags = (1 if continue_run else 0) | (2 if per_replica else 0) | (4 if resident else 0) | (8 if per_group else 0)
        sweeps = int(num_sweeps) if per_replica else (betas.shape[1] if per_group else len(betas))
        init = None
        if initial_states is not None:
            init = np.ascontiguousarray(initial_states, dtype=self.state_dtype)
            if init.shape != (num_reads, self.n):
                raise ValueError("initial_states must have shape (num_reads, n) = (%d, %d)"
                                 % (num_reads, self.n))
            if self._inv is not None:
                dev = np.zeros((num_reads, self.n_dev), dtype=self.state_dtype)
                dev[:, self._inv] = init
                init = dev
        _lib.call("mi_sa_anneal_ex", self._handle(), int(num_reads), C.c_uint32(int(replica_offset) & 0xFFFFFFFF), sweeps,
                  betas, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), init, int(resync_interval),
                  C.c_uint32(int(sweep_offset) & 0xFFFFFFFF), C.c_uint32(flags))
        self._last = (int(num_reads), sweeps)

    # -- parallel tempering: exchange step on the device (K6) ----------------------------------------
    def tempering_begin(self, ladder_betas, chains: int, first_replica: int, num_local: int):
        lad = np.ascontiguousarray(ladder_betas, dtype=np.float64)
        self._pt_total = len(lad) * int(chains)
        _lib.call("mi_sa_tempering_begin", self._handle(), lad, len(lad), int(chains), C.c_uint32(int(first_replica)),
                  int(num_local))

    def tempering_exchange(self, rnd: int, seed: int, all_energies: Optional[np.ndarray] = None):
        """Neighbouring rungs of every chain exchange (Metropolis on a counter-based stream of (seed, round)).
        ``all_energies`` = None when this GPU owns every replica (nothing leaves HBM), else the all-gathered
        energies of the run in global replica order."""
        en = None if all_energies is None else np.ascontiguousarray(all_energies, dtype=np.float64)
        if en is not None and len(en) != self._pt_total:
            raise ValueError("all_energies must hold the %d energies of the run" % self._pt_total)
        _lib.call("mi_sa_tempering_exchange", self._handle(), C.c_uint32(int(rnd) & 0xFFFFFFFF),
                  C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), en)

    def tempering_exchange_device(self, rnd: int, seed: int, all_energies_dev):
        """The same exchange with the all-gathered energies already in HBM: ``all_energies_dev`` = a contiguous float64
        torch tensor on this problem's GPU (the output of the RCCL all-gather), read in place."""
        if all_energies_dev.numel() != self._pt_total or not all_energies_dev.is_contiguous():
            raise ValueError("all_energies_dev must hold the %d energies of the run, contiguous" % self._pt_total)
        _lib.call("mi_sa_tempering_exchange_dev", self._handle(), C.c_uint32(int(rnd) & 0xFFFFFFFF),
                  C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), all_energies_dev.data_ptr())

    def device_energies(self):
        """The energies of the last run as a float64 torch tensor that ALIASES the library's HBM buffer (no copy;
        waits for the run; valid until the next anneal on this handle): the send buffer of a GPU-to-GPU collective."""
        import torch
        d_en, R = C.c_void_p(), C.c_int(0)
        _lib.call("mi_sa_device_results", self._handle(), None, d_en, R)

        class _Alias:                     # the array-interface protocol torch.as_tensor understands for device memory
            __cuda_array_interface__ = {"shape": (int(R.value),), "typestr": "<f8", "data": (int(d_en.value), False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_Alias(), device=torch.device("cuda", self.device))

    def tempering_state(self):
        """``(rung of every replica of the run, exchanges proposed, exchanges accepted)``."""
        rung = np.empty(self._pt_total, dtype=np.int32)
        prop, acc = C.c_uint64(0), C.c_uint64(0)
        _lib.call("mi_sa_tempering_state", self._handle(), rung, prop, acc)
        return rung.astype(np.int64), int(prop.value), int(acc.value)

    def sync(self):
        _lib.call("mi_sa_sync", self._handle())

    def kernel_ms(self) -> float:
        return _lib.call_ms("mi_sa_last_kernel_ms", self._handle())

    def label_agreement(self, groups: Optional[int] = None) -> dict:
        """ARI and NMI of every pair r < s of the last run's replicas inside each group of consecutive replicas (``groups``
        None: the problem's own resolution groups), computed on the states in HBM without a host copy; hole seats are
        not cells.  Potts problems only.  Returns ``ari``, ``nmi`` (fp64) and ``pair_sum`` (int64), each of shape
        (groups, C(R / groups, 2)) in row-major pair order, and ``kernel_ms``.  Leaves the run untouched."""
        if self._last is None:
            raise RuntimeError("label_agreement() before anneal()")
        R = self._last[0]
        G = self.groups if groups is None else int(groups)
        if G < 1 or R % G:
            raise ValueError("%d replicas do not split into %d equal groups" % (R, G))
        P = (R // G) * (R // G - 1) // 2
        ari, nmi = np.empty((G, P)), np.empty((G, P))
        S = np.empty((G, P), dtype=np.int64)
        ms = _lib.call_ms("mi_sa_problem_label_agreement", self._handle(), G, ari, nmi, S)
        return {"ari": ari, "nmi": nmi, "pair_sum": S, "kernel_ms": ms}

    def coassociation(self, groups: Optional[int] = None, ref=None, edges=None, matrix: bool = False,
                      hist: bool = True) -> dict:
        """Co-association of the last run's replicas inside each group of consecutive replicas (``groups`` None: the
        problem's own resolution groups), computed on the states in HBM without a host copy: what
        ``metrics.coassociation(fetch()[0], groups, ref, edges, matrix, hist=hist)`` returns, in the caller's variable order (hole
        seats are not cells).  ``ref`` labels must lie in [0, 64).  Potts problems only.  Leaves the run untouched."""
        from .metrics import _coassoc_outputs, _coassoc_result, _edge_arrays
        if self._last is None:
            raise RuntimeError("coassociation() before anneal()")
        R = self._last[0]
        G = self.groups if groups is None else int(groups)
        if G < 1 or R % G:
            raise ValueError("%d replicas do not split into %d equal groups" % (R, G))
        Rg, n, nd = R // G, self.n, self.n_dev
        cols = np.arange(n) if self._inv is None else np.asarray(self._inv)
        dref, Kref = None, None
        if ref is not None:
            r = np.asarray(ref)
            r = np.broadcast_to(r[None, :], (G, r.shape[0])) if r.ndim == 1 else r
            if r.shape != (G, n) or not np.issubdtype(r.dtype, np.integer) or r.min() < 0 or r.max() >= 64:
                raise ValueError("ref must be (n,) or (groups, n) integer labels in [0, 64)")
            Kref = int(r.max()) + 1
            dref = np.zeros((G, nd), dtype=np.uint16)
            dref[:, cols] = r
        eu = ev = None
        if edges is not None:
            eu, ev = _edge_arrays(edges, n)
            eu = np.ascontiguousarray(cols[eu], dtype=np.int32)
            ev = np.ascontiguousarray(cols[ev], dtype=np.int32)
        hist, rowsum, edge, counts = _coassoc_outputs(G, Rg, nd, Kref, None if eu is None else len(eu), matrix, hist)
        ms = _lib.call_ms("mi_sa_problem_coassociation", self._handle(), G, dref, int(Kref or 1), eu, ev,
                          0 if eu is None else len(eu), hist, rowsum, edge, counts)
        if nd != n or self._inv is not None:             # device columns -> the caller's variables
            rowsum = None if rowsum is None else np.ascontiguousarray(rowsum[:, cols])
            counts = None if counts is None else np.ascontiguousarray(counts[:, cols][:, :, cols])
        return _coassoc_result(G, Rg, hist, rowsum, edge, counts, ms)

    def components(self):
        """Every cluster of every replica of the last run split into its connected components in the model's graph (the
        stored couplings), computed on the states and the adjacency in HBM without a host copy: what
        ``metrics.split_disconnected((rowptr, col), n, fetch()[0])`` returns, ``(labels int32 (R, n), counts (R,))`` in
        the caller's variable order, numbered by smallest cell (hole seats are not cells).  Potts problems only.  Leaves
        the run untouched."""
        from .metrics import renumber_by_first_cell
        if self._last is None:
            raise RuntimeError("components() before anneal()")
        R = self._last[0]
        out = np.empty((R, self.n_dev), dtype=np.int32)
        cnt = np.empty(R, dtype=np.int32)
        _lib.call("mi_sa_problem_components", self._handle(), out, cnt, None)
        if self._inv is not None:                        # device columns -> the caller's variables, numbered in their order
            out = renumber_by_first_cell(np.take(out, self._inv, axis=1))
        return out, cnt

    def launch_count(self) -> int:
        """Kernel launches that served the last anneal (kernel_ms() / launch_count() = mean launch time)."""
        k = C.c_int(0)
        _lib.call("mi_sa_last_launch_count", self._handle(), k)
        return int(k.value)

    def kernel_name(self) -> str:
        """The kernel(s) that served the last anneal, as a profiler names them."""
        buf = C.create_string_buffer(256)
        _lib.call("mi_sa_last_kernel_name", self._handle(), buf, 256)
        return buf.value.decode()

    def adjacency_bytes_per_slot(self) -> int:
        """Packed adjacency bytes one wavefront fetched per 64-variable slot in the last anneal (which packing the pair
        kernel read: 6144 / 6400 / 12544 with 16-bit neighbour words, 7936 / 8448 / 16640 without); 0 for other kernels."""
        k = C.c_int(0)
        _lib.call("mi_sa_last_adjacency_bytes_per_slot", self._handle(), k)
        return int(k.value)

    def fetch(self, states: bool = True, energies: bool = True):
        if self._last is None:
            raise RuntimeError("fetch() before anneal()")
        R = self._last[0]
        st = np.empty((R, self.n_dev), dtype=self.state_dtype) if states else None
        en = np.empty(R, dtype=np.float64) if energies else None
        stats = np.zeros(3, dtype=np.uint64)
        _lib.call("mi_sa_fetch", self._handle(), st, en, stats)
        info = {"proposals": int(R) * int(self._last[1]) * int(self.n),
                "accepted": int(stats[1]), "row_bytes": int(stats[2])}
        if st is not None and self._inv is not None:
            # caller's variable i sits in device column inv[i]: a column gather (np.take is the fast form)
            st = np.take(st, self._inv, axis=1)
        return st, en, info

    def best(self, want_state: bool = True):
        idx = C.c_int(0)
        en = C.c_double(0.0)
        key = C.c_uint64(0)
        st = np.empty(self.n_dev, dtype=self.state_dtype) if want_state else None
        _lib.call("mi_sa_best", self._handle(), idx, en, key, st)
        if st is not None and self._inv is not None:
            st = st[self._inv]
        return int(idx.value), float(en.value), int(key.value), st


def weighted_layout_csr(rowptr, col, val, lin, weights, energy_model=None):
    """The device-side model of a structured binary model with pair-term weights (host work only): the unit-weight
    variables as usual (64-seat slots free of internal edges, models.padded_slot_layout), the others -- few, no sparse
    couplings -- in one more slot.  Returns ``(rowptr, col, val, lin, weights, seats, n_dev, val64, lin64)``, the first
    five in device order (holes: lin = +inf, weight 1), ``seats[i]`` the device column of the caller's variable i."""
    from .models import pad_csr, padded_slot_layout
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    weights = np.asarray(weights, dtype=np.int64)
    n_caller = len(lin)
    deg = np.diff(rowptr)
    heavy = np.flatnonzero(weights != 1)
    light = np.flatnonzero(weights == 1)
    if np.any(weights < 1) or len(heavy) > 64 or np.any(deg[heavy] != 0):
        raise ValueError("pair-term weights: positive integers; at most 64 variables with a weight other than 1, "
                         "and those without sparse couplings")
    # the layout of the unit-weight variables alone (the others have no edges): their CSR renumbered 0 .. len(light) - 1
    renum = np.full(n_caller, -1, dtype=np.int64)
    renum[light] = np.arange(len(light))
    rp_l = np.concatenate([[0], np.cumsum(deg[light])]).astype(np.int32)
    keep = np.repeat(weights == 1, deg)
    seats_l, nslots, _ = padded_slot_layout(rp_l, renum[col[keep]].astype(np.int32), slot=64)
    seats = np.empty(n_caller, dtype=np.int64)
    seats[light] = seats_l
    seats[heavy] = nslots * 64 + np.arange(len(heavy))
    n_dev = (nslots + 1) * 64
    val64 = lin64 = None
    if energy_model is not None:
        val64, lin64 = np.asarray(energy_model[0], dtype=np.float64), np.asarray(energy_model[1], dtype=np.float64)
        rp, cc, vv, val64 = pad_csr(rowptr, col, val, seats, n_dev, also=val64)
        l64 = np.zeros(n_dev, dtype=np.float64)
        l64[seats] = lin64
        lin64 = l64
    else:
        rp, cc, vv = pad_csr(rowptr, col, val, seats, n_dev)
    lpad = np.full(n_dev, np.inf, dtype=np.float32)
    lpad[seats] = np.asarray(lin, dtype=np.float32)
    wdev = np.ones(n_dev, dtype=np.int32)
    wdev[seats] = weights
    return (np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(cc, dtype=np.int32),
            np.ascontiguousarray(vv, dtype=np.float32), lpad, wdev, seats, n_dev, val64, lin64)


def plan_anneal(kind, rowptr, col, n, num_reads, num_cases=2, cus=0, options=None, pair_weight_slot=-1,
                node_weights=False, min_cluster_size=0):
    """Which kernel an anneal of ``num_reads`` replicas would run for a structured model (``kind``: _lib.KIND_CSR_RANK1
    or KIND_POTTS_CSR; the device-side CSR), decided on the host without touching a device (mi_sa_plan_anneal).
    ``cus``: compute units of the device (0: 256); ``options``: ``{key: value}`` (or ``"key=value,..."``) with the
    k2_* / k3_* keys of ``Problem.set_option``.  Returns ``(kernel_name, adjacency_bytes_per_slot)``; raises MiSaError
    with the code and message that creating or annealing the problem would."""
    if isinstance(options, dict):
        options = ",".join("%s=%d" % (k, int(v)) for k, v in sorted(options.items()))
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    name = C.create_string_buffer(256)
    nbytes = C.c_int(0)
    _lib.call("mi_sa_plan_anneal", int(kind), rowptr, col, int(n), int(num_cases), int(num_reads), int(cus),
              (options or "").encode(), int(pair_weight_slot), int(bool(node_weights)), int(min_cluster_size), name, 256,
              nbytes)
    return name.value.decode(), int(nbytes.value)


def plan_dense(n, num_reads, num_sweeps, resync_interval=0, per_replica=False, cus=0, resident_waves=4096, options=None):
    """Which kernel(s) an anneal of a dense model of ``n`` variables would run, and in how many launches, decided on the
    host without touching a device (mi_sa_plan_dense).  ``per_replica``: one temperature per replica (``anneal`` with
    ``num_sweeps``); ``cus``: compute units of the device (0: 256); ``resident_waves``: co-resident wavefronts of the
    wave-per-replica kernel (read only where it serves the run); ``options``: ``{key: value}`` (or ``"key=value,..."``)
    with the dense keys of ``Problem.set_option``.  Returns ``(kernel_name, launch_count, field_bytes)`` -- the name up to
    the hand-over of a cooling run, which is measured; raises MiSaError with the code and message the anneal would."""
    if isinstance(options, dict):
        options = ",".join("%s=%d" % (k, int(v)) for k, v in sorted(options.items()))
    name = C.create_string_buffer(256)
    launches, nbytes = C.c_int(0), C.c_uint64(0)
    _lib.call("mi_sa_plan_dense", int(n), int(num_reads), int(num_sweeps), int(resync_interval),
              C.c_uint32(2 if per_replica else 0), int(cus), int(resident_waves), (options or "").encode(), name, 256, launches,
              nbytes)
    return name.value.decode(), int(launches.value), int(nbytes.value)


def energy_dense(Qs: np.ndarray, X: np.ndarray, offset: float = 0.0, device: int = 0, path: int = 0,
                 return_ms: bool = False):
    """Batched ``E_r = x_r^T Qs x_r + offset`` on the GPU (kernel K4).  ``path``: 0 auto (MFMA for
    batches of >= 32 states), 1 exact-fp64 VALU, 2 f32-input MFMA.  ``X`` holds 0 / 1; any other value after the cast to
    uint8 (a -1 spin becomes 255) is refused by the library."""
    Qs = np.ascontiguousarray(Qs, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.uint8)
    if X.ndim != 2 or X.shape[1] != Qs.shape[0]:
        raise ValueError("X must have shape (R, n)")
    out = np.empty(X.shape[0], dtype=np.float64)
    ms = _lib.call_ms("mi_energy_dense_f32_ex", Qs, Qs.shape[0], X, X.shape[0], float(offset), out, int(device), int(path))
    return (out, ms) if return_ms else out


def energy_dense_f64(Qs: np.ndarray, X: np.ndarray, offset: float = 0.0, device: int = 0) -> np.ndarray:
    """``E_r = x_r^T Qs x_r + offset`` over an fp64 matrix on the GPU (every entry added once into fp64): the
    caller-model energies of a dense problem's samples."""
    Qs = np.ascontiguousarray(Qs, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.uint8)
    if X.ndim != 2 or Qs.ndim != 2 or Qs.shape[0] != Qs.shape[1] or X.shape[1] != Qs.shape[0]:
        raise ValueError("Qs must be n x n and X must have shape (R, n)")
    out = np.empty(X.shape[0], dtype=np.float64)
    _lib.call("mi_energy_dense_f64", Qs, Qs.shape[0], X, X.shape[0], float(offset), out, int(device))
    return out
