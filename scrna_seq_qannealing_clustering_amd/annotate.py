"""Reference-based cell-type annotation (the reference notebook's ``SingleR(test, ref, labels)`` step) on the GPU.

The chain is this package's specification ("chain A"), modelled on SingleR's defaults
(``de.method = "classic"``, ``quantile = 0.8``, ``fine.tune = TRUE``, ``tune.thresh = 0.05``, ``prune = TRUE``); agreement
with R's SingleR is not pinned.

    common genes (host) -> classic markers (host fp64) -> Spearman scores on the markers, 0.8 quantile per label (device)
    -> fine-tuning per cell (device) -> pruning (host fp64)

The device work is include/mi_annot.h (csrc/annot_kernels.hip): the reference is uploaded and ranked once into a handle, the
test cells are densified on the marker genes and scored in chunks of at most ``MAX_CHUNK`` cells.  There is no CPU path.

The cells may also be an open ``preprocess.ExpressionMatrix``: its marker columns are then gathered on the device, chunk by
chunk, and no n x g matrix crosses the host (``single_r(handle, ...)``, ``handle.annotate(...)``).  ``clusters=`` annotates
one mean profile per cluster instead of every cell (SingleR's ``clusters =``), the means being one device reduction over
the handle (:func:`cluster_means`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

MAX_GENES, MAX_LABELS, MAX_SAMPLES, MAX_CHUNK = 8191, 64, 4096, 16384      # include/mi_annot.h
QUANTILE, TUNE_THRESH, PRUNE_NMADS = 0.8, 0.05, 3.0
MI_ESTATE = -6                                                             # include/mi_sa.h: a call out of order


# ---- host steps -----------------------------------------------------------------------------------------------------------

def encode_labels(labels):
    """-> (ids int32, values): label ids in order of first appearance, and the label value of each id."""
    index, ids = {}, np.empty(len(labels), dtype=np.int32)
    for i, v in enumerate(labels):
        v = v.item() if isinstance(v, np.generic) else v
        ids[i] = index.setdefault(v, len(index))
    return ids, list(index)


def default_de_n(L: int) -> int:
    """markers kept per ordered pair of labels: round(500 * (2/3) ** log2(L))"""
    return int(round(500.0 * (2.0 / 3.0) ** math.log2(L)))


def label_medians(R, ids, L: int):
    """(L, g) fp64: ``np.median`` of every gene over each label's samples"""
    R = np.asarray(R, dtype=np.float64)
    return np.stack([np.median(R[ids == l], axis=0) for l in range(L)])


def markers_from_medians(med, de_n=None):
    """Step 2 on the (L, g) medians.  For every ordered pair a != b the ``de_n`` genes with the largest
    ``med[a] - med[b]``, ties to the lower gene index, of which only strictly positive differences are kept.
    -> (pairs, M): ``pairs[(a, b)]`` the pair's genes in that order, ``M`` the sorted union."""
    med = np.asarray(med, dtype=np.float64)
    L = med.shape[0]
    n = default_de_n(L) if de_n is None else int(de_n)
    if n < 1:
        raise ValueError("de_n must be >= 1 (got %d)" % n)
    pairs = {}
    for a in range(L):
        for b in range(L):
            if a == b:
                continue
            d = med[a] - med[b]
            top = np.argsort(-d, kind="stable")[:n]
            pairs[(a, b)] = top[d[top] > 0.0].astype(np.int64)
    M = np.unique(np.concatenate(list(pairs.values()))) if pairs else np.empty(0, dtype=np.int64)
    return pairs, M.astype(np.int64)


def classic_markers(R, labels, de_n=None):
    """Step 2 on a reference matrix (S samples x g genes) and its labels (any hashable; ids follow first appearance).
    -> (pairs, M) as :func:`markers_from_medians`."""
    ids, values = encode_labels(labels)
    R = np.asarray(R, dtype=np.float64)
    if R.ndim != 2 or R.shape[0] != len(ids):
        raise ValueError("R must be (S, g) with one label per sample (got %s, %d labels)" % (R.shape, len(ids)))
    return markers_from_medians(label_medians(R, ids, len(values)), de_n)


def quantile(c, q: float = QUANTILE) -> float:
    """the q quantile of the values c by linear interpolation between order statistics, as written in the specification"""
    c = np.sort(np.asarray(c, dtype=np.float64))
    s = c.size
    pos = q * (s - 1)
    lo = int(math.floor(pos))
    return float(c[lo] + (pos - lo) * (c[min(lo + 1, s - 1)] - c[lo]))


def common_genes(test_names, ref_names):
    """Step 1.  -> (test_idx, ref_idx): the genes in both lists, in the test list's order.  A duplicate name is an error."""
    def positions(names, what):
        pos = {}
        for i, g in enumerate(names):
            if g in pos:
                raise ValueError("duplicate gene name %r in the %s gene names" % (g, what))
            pos[g] = i
        return pos
    positions(test_names, "test")
    ref_pos = positions(ref_names, "reference")
    test_idx = [i for i, g in enumerate(test_names) if g in ref_pos]
    ref_idx = [ref_pos[test_names[i]] for i in test_idx]
    return np.asarray(test_idx, dtype=np.int64), np.asarray(ref_idx, dtype=np.int64)


def prune_scores(scores, labels, tuned_best=None, tuned_next=None, nmads: float = PRUNE_NMADS):
    """Step 5.  ``scores`` (n, L) of step 3, ``labels`` (n,) the final label ids.  delta = max - median of a cell's scores; a
    cell is pruned when its delta is below median - nmads * 1.4826 * MAD of the deltas of the cells sharing its label, or
    when ``tuned_best - tuned_next < 0``.  -> (delta, pruned)"""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    delta = scores.max(axis=1) - np.median(scores, axis=1)
    pruned = np.zeros(scores.shape[0], dtype=bool)
    for l in np.unique(labels):
        sel = labels == l
        d = delta[sel]
        med = np.median(d)
        mad = np.median(np.abs(d - med))
        pruned[sel] = d < med - nmads * 1.4826 * mad
    if tuned_best is not None and tuned_next is not None:
        pruned |= (np.asarray(tuned_best, dtype=np.float64) - np.asarray(tuned_next, dtype=np.float64)) < 0.0
    return delta, pruned


def pair_masks(pairs, M, L: int):
    """the pair-marker lists as bit masks over M: (L * L, ceil(m / 32)) uint32, bit j of row a * L + b for M[j] in pairs[(a, b)]"""
    m = len(M)
    masks = np.zeros((L * L, (m + 31) // 32), dtype=np.uint32)
    for (a, b), genes in pairs.items():
        j = np.searchsorted(M, genes)
        np.bitwise_or.at(masks[a * L + b], j >> 5, (np.uint32(1) << (j & 31).astype(np.uint32)))
    return masks


class Reference:
    """A labelled reference: ``R`` (S samples x g genes, log-scale, finite), its gene names and one label per sample (any
    hashable, L distinct; ids follow first appearance).  Holds the per-label medians; the markers depend on which genes the
    test matrix shares with it and are kept per gene subset."""

    def __init__(self, R, gene_names, labels, de_n=None):
        self.R = np.ascontiguousarray(R, dtype=np.float32)
        self.gene_names = list(gene_names)
        if self.R.ndim != 2 or self.R.shape[1] != len(self.gene_names):
            raise ValueError("R must be (S, g) with g gene names (got %s, %d names)" % (self.R.shape, len(self.gene_names)))
        if len(labels) != self.R.shape[0]:
            raise ValueError("one label per reference sample: %d labels, %d samples" % (len(labels), self.R.shape[0]))
        if not np.isfinite(self.R).all():
            raise ValueError("the reference matrix holds a NaN or an infinity")
        self.label_ids, self.label_values = encode_labels(labels)
        self.L = len(self.label_values)
        self.de_n = default_de_n(self.L) if de_n is None else int(de_n)
        self.medians = label_medians(self.R, self.label_ids, self.L)
        self._cache = {}

    def markers_on(self, ref_idx=None):
        """(pairs, M) among the reference genes ``ref_idx`` (all by default); indices are positions in ``ref_idx``"""
        key = None if ref_idx is None else np.asarray(ref_idx, dtype=np.int64).tobytes()
        if key not in self._cache:
            med = self.medians if ref_idx is None else self.medians[:, ref_idx]
            self._cache = {key: markers_from_medians(med, self.de_n)}
        return self._cache[key]

    @property
    def markers(self):
        return self.markers_on(None)


# ---- the device handle ----------------------------------------------------------------------------------------------------

def _which(which: str) -> int:
    """0 for the ``"counts"`` of an expression handle, 1 for its ``"normalized"`` matrix"""
    if which not in ("counts", "normalized"):
        raise ValueError("which must be 'counts' or 'normalized' (got %r)" % (which,))
    return int(which == "normalized")


class Annotator(_lib.Handle):
    """mi_annot: a reference restricted to m marker genes (``R`` S x m), its label ids in [0, L) and the pair masks,
    resident and ranked on the device.  ``score`` takes a chunk of cells (n_c x m), ``fine_tune`` works on that chunk."""
    _destroy = "mi_annot_destroy"

    def __init__(self, R, label_ids, L: int, masks=None, device: int = 0):
        R = np.ascontiguousarray(R, dtype=np.float32)
        ids = np.ascontiguousarray(label_ids, dtype=np.int32)
        if R.ndim != 2 or ids.shape != (R.shape[0],):
            raise ValueError("R must be (S, m) with S label ids (got %s, %s)" % (R.shape, ids.shape))
        self.S, self.m, self.L = R.shape[0], R.shape[1], int(L)
        W = (self.m + 31) // 32
        if masks is None:
            masks = np.zeros((max(self.L, 0) ** 2, W), dtype=np.uint32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        if masks.shape != (max(self.L, 0) ** 2, W):
            raise ValueError("masks must be (L * L, ceil(m / 32)) = (%d, %d) (got %s)" % (self.L ** 2, W, masks.shape))
        h = C.c_void_p()
        self.rank_ref_ms = _lib.call_ms("mi_annot_create", R, self.S, self.m, ids, self.L, masks, int(device), h)
        self._h = h
        self.n_c = 0

    def score(self, X, integers: bool = False) -> dict:
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.m:
            raise ValueError("X must be (n_c, %d) (got %s)" % (self.m, X.shape))
        n = X.shape[0]
        outs = self._outputs(n, integers)
        ms = (C.c_float * 3)()
        self.n_c = 0
        _lib.call("mi_annot_score", self._handle(), X, n, *outs, ms)
        self.n_c = n
        return self._result(outs, {"rank": ms[0], "cross": ms[1], "scores": ms[2]}, integers)

    def _outputs(self, n: int, integers: bool):
        """the five host outputs of a scoring call on n rows, in the order of the C prototypes (None where not asked for)"""
        sab = np.empty((n, self.S), dtype=np.int64) if integers else None
        sa2 = np.empty(n, dtype=np.int64) if integers else None
        sb2 = np.empty(self.S, dtype=np.int64) if integers else None
        return sab, sa2, sb2, np.empty((n, self.L), dtype=np.float64), np.empty(n, dtype=np.int32)

    @staticmethod
    def _result(outs, ms: dict, integers: bool) -> dict:
        sab, sa2, sb2, scores, first = outs
        out = {"scores": scores, "first_labels": first, "kernel_ms": {k: float(v) for k, v in ms.items()}}
        if integers:
            out.update(sab=sab, sa2=sa2, sb2=sb2)
        return out

    def _cols(self, handle, cols):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if cols.shape != (self.m,):
            raise ValueError("cols must hold the handle's positions of the %d marker genes (got shape %s)" % (self.m, cols.shape))
        return cols

    def score_matrix(self, handle, cols, i0: int, i1: int, which: str = "normalized", integers: bool = False) -> dict:
        """:meth:`score` on the cells ``i0 .. i1 - 1`` of an open ``preprocess.ExpressionMatrix`` (dense or sparse),
        restricted to its genes ``cols`` (m indices, no repeats), gathered on the device: the ``"counts"`` (the uploaded
        values) or the ``"normalized"`` matrix.  The same dict, bit for bit that of ``score`` on the densified slice;
        ``kernel_ms`` gains ``gather``.  The handle is not modified."""
        w = _which(which)
        cols = self._cols(handle, cols)
        n = int(i1) - int(i0)
        outs = self._outputs(max(n, 0), integers)
        ms = (C.c_float * 4)()
        self.n_c = 0
        _lib.call("mi_annot_score_matrix", self._handle(), handle._handle(), w, cols, int(i0), n, *outs, ms)
        self.n_c = n
        return self._result(outs, dict(zip(("gather", "rank", "cross", "scores"), ms)), integers)

    def score_clusters(self, handle, cols, cluster_of, K: int, which: str = "normalized", integers: bool = False) -> dict:
        """:meth:`score` on K rows, row c the mean profile on the genes ``cols`` of the handle's cells with
        ``cluster_of[i] == c`` (ids in [0, K), every id used): the fp64 sum in ascending cell index, divided by the size,
        rounded to fp32.  Also returns ``sizes`` (K,); ``kernel_ms`` gains ``means``."""
        w = _which(which)
        cols = self._cols(handle, cols)
        of = np.ascontiguousarray(cluster_of, dtype=np.int32)
        if of.shape != (handle.n,):
            raise ValueError("cluster_of must hold one cluster id per cell of the handle (%d; got shape %s)" % (handle.n, of.shape))
        K = int(K)
        outs = self._outputs(max(K, 0), integers)
        sizes = np.empty(max(K, 0), dtype=np.int32)
        ms = (C.c_float * 4)()
        self.n_c = 0
        _lib.call("mi_annot_score_clusters", self._handle(), handle._handle(), w, cols, of, K, sizes, *outs, ms)
        self.n_c = K
        out = self._result(outs, dict(zip(("means", "rank", "cross", "scores"), ms)), integers)
        out["sizes"] = sizes
        return out

    def fetch_chunk(self) -> np.ndarray:
        """the resident chunk as the chain reads it, (n_c, m) float32: the cells of the last ``score`` / ``score_matrix``,
        or the K mean rows of the last ``score_clusters``"""
        if self.n_c < 1:
            raise _lib.MiSaError(MI_ESTATE, "no chunk is resident: the last scoring call was refused, or none has run")
        out = np.empty((self.n_c, self.m), dtype=np.float32)
        _lib.call("mi_annot_fetch_chunk", self._handle(), out)
        return out

    def fine_tune(self) -> dict:
        """the fine-tuning loop on the chunk of the last ``score`` call; after a ``score`` that raised there is none"""
        n = self.n_c
        if n < 1:                                   # the outputs below are sized by n: never hand the library empty ones
            raise _lib.MiSaError(MI_ESTATE, "score() has not run, or its last call was refused: no chunk is resident")
        labels, iters = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        best, nxt = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        ms = _lib.call_ms("mi_annot_fine_tune", self._handle(), labels, best, nxt, iters)
        return {"labels": labels, "tuned_best": best, "tuned_next": nxt, "iterations": iters,
                "kernel_ms": {"fine_tune": ms}}


def _chunks(n: int, chunk: int):
    chunk = int(chunk)
    if chunk < 1 or chunk > MAX_CHUNK:
        raise ValueError("chunk must be in [1, %d] (got %d)" % (MAX_CHUNK, chunk))
    return [(i, min(i + chunk, n)) for i in range(0, n, chunk)]


def _add_ms(total, part):
    for k, v in part.items():
        total[k] = total.get(k, 0.0) + v


def _best_two(scores):
    """largest and second-largest entry per row (-inf when there is only one)"""
    s = np.sort(scores, axis=1)
    return s[:, -1].copy(), (s[:, -2].copy() if s.shape[1] > 1 else np.full(s.shape[0], -np.inf))


def _run(ann: Annotator, score_of, n: int, chunk: int, fine_tune: bool, integers: bool) -> dict:
    """every chunk through the handle; score_of(i0, i1) -> the result of one of ``ann``'s scoring calls on the cells
    i0 .. i1 - 1 (which stay resident for the fine-tuning)"""
    parts, ms = [], {"rank_ref": ann.rank_ref_ms}
    for i0, i1 in _chunks(n, chunk):
        r = score_of(i0, i1)
        _add_ms(ms, r.pop("kernel_ms"))
        if fine_tune:
            t = ann.fine_tune()
            _add_ms(ms, t.pop("kernel_ms"))
            r.update(t)
        parts.append(r)
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "sb2"}
    if integers:
        out["sb2"] = parts[0]["sb2"]
    ms["total"] = sum(ms.values())
    out["kernel_ms"] = ms
    return out


def score_pass(X, R, labels=None, masks=None, fine_tune: bool = False, device: int = 0, chunk: int = MAX_CHUNK) -> dict:
    """The device passes on explicit matrices, for tests.  ``X`` (n, m) cells and ``R`` (S, m) samples on the same m genes,
    ``labels`` (S,) label ids in [0, L) with L = max + 1 (all one label by default), ``masks`` as :func:`pair_masks` (no
    markers by default).  Returns the exact integers of step 3, ``sab`` (n, S) = sum a b, ``sa2`` (n,) = sum a^2, ``sb2``
    (S,) = sum b^2 of the doubled midranks, the ``scores`` (n, L) and ``first_labels`` (n,); with ``fine_tune`` also ``labels``,
    ``tuned_best``, ``tuned_next``, ``iterations``; and ``kernel_ms`` per pass."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    R = np.ascontiguousarray(R, dtype=np.float32)
    if X.ndim != 2 or R.ndim != 2 or X.shape[1] != R.shape[1]:
        raise ValueError("X must be (n, m) and R (S, m) (got %s, %s)" % (X.shape, R.shape))
    ids = np.zeros(R.shape[0], dtype=np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    L = int(ids.max()) + 1 if ids.size else 0
    with Annotator(R, ids, L, masks, device=device) as ann:
        return _run(ann, lambda i0, i1: ann.score(X[i0:i1], integers=True), X.shape[0], chunk, fine_tune, True)


def _marker_setup(names, ref: Reference):
    """steps 1 and 2 for a test matrix with the gene names ``names`` -> (cols, annotator arguments): the test-side positions
    of the marker genes M, and ``(R on M, label ids, L, pair masks)``"""
    test_idx, ref_idx = common_genes(names, ref.gene_names)
    pairs, M = ref.markers_on(ref_idx)
    if len(M) < 1:
        raise ValueError("no marker genes: the reference needs at least two labels whose medians differ on the %d common genes"
                         % len(test_idx))
    if len(M) > MAX_GENES:
        raise ValueError("%d marker genes exceed %d: lower de_n" % (len(M), MAX_GENES))
    return test_idx[M], (ref.R[:, ref_idx[M]], ref.label_ids, ref.L, pair_masks(pairs, M, ref.L))


def single_r(X, gene_names, ref: Reference, fine_tune: bool = True, prune: bool = True, device: int = 0,
             chunk: int = MAX_CHUNK, which: str = "normalized", clusters=None) -> dict:
    """Annotate the cells of ``X`` (n cells x g genes, with its ``gene_names``) against ``ref``.  ``X`` is a dense array or
    a ``scipy.sparse`` matrix of log-normalised values, such as ``preprocess.log_normalize`` returns, or an open
    ``preprocess.ExpressionMatrix`` (dense or sparse; also the ``corrected`` handle of ``sctransform(...,
    return_corrected=True)``), whose ``which`` matrix (``"normalized"``, the output of ``normalize()`` or the ``data`` slot,
    or ``"counts"``, the uploaded values) is read where it is: the marker columns are gathered on the device and nothing of
    the n x g matrix crosses the host.  ``"normalized"`` before ``normalize()`` raises the library's ``MI_ESTATE``.  ``which``
    is used for a handle only, which is annotated on its own device.

    Returns ``labels`` (after fine-tuning), ``first_labels`` (the argmax of the scores) and ``pruned_labels`` (``None``
    where pruned) as the reference's own label values (object arrays); ``scores`` (n, L) with the columns in the order of
    ``label_values``; ``tuned_best``, ``tuned_next``, ``iterations``, ``delta``; ``marker_genes`` (the names of M);
    ``label_ids`` (the final label ids) and ``kernel_ms`` per pass (with ``gather`` for a handle).  A sparse ``X`` is
    densified on the marker genes chunk by chunk (``chunk`` cells, at most ``MAX_CHUNK``), so memory stays bounded for any n.

    ``clusters`` (SingleR's ``clusters =``): one cluster label per cell, any hashable values.  The K clusters are annotated
    instead of the cells, each as the mean profile of its cells on the marker genes (the fp64 sum in cell order, divided by
    the size, rounded to fp32; one device reduction for every kind of ``X``): every per-row result then has K rows, in the
    order of ``cluster_values`` (first appearance), and the pruning runs over the K rows, as SingleR's does.  Also returned:
    ``cluster_values``, ``cluster_sizes`` and ``cell_labels``, each cell's cluster's label (n,), what
    ``plot_and_save_embedding`` takes.  A host ``X`` is uploaded as it is into a temporary ``ExpressionMatrix`` and read as
    its ``"counts"``: its values must be non-negative and finite, as ``find_all_markers`` requires of sparse input."""
    from . import preprocess
    names = list(gene_names)
    on_handle = isinstance(X, preprocess.ExpressionMatrix)
    shape = (X.n, X.g) if on_handle else tuple(X.shape)
    if len(shape) != 2 or shape[1] != len(names):
        raise ValueError("X must be (n, g) with g gene names (got %s, %d names)" % (shape, len(names)))
    _which(which)
    n = rows = shape[0]
    if clusters is not None:
        if len(clusters) != n:
            raise ValueError("clusters must hold one label per cell: %d labels, %d cells" % (len(clusters), n))
        cluster_ids, cluster_values = encode_labels(clusters)
        rows = len(cluster_values)
        if rows > MAX_CHUNK:
            raise ValueError("%d clusters exceed %d" % (rows, MAX_CHUNK))
    cols, ref_args = _marker_setup(names, ref)
    if on_handle:
        device = X.device
    if clusters is not None:
        handle = X if on_handle else preprocess.ExpressionMatrix(X, device=device)
        try:
            with Annotator(*ref_args, device=device) as ann:
                score_of = lambda i0, i1: ann.score_clusters(handle, cols, cluster_ids, rows, which if on_handle else "counts")
                out = _run(ann, score_of, rows, MAX_CHUNK, fine_tune, False)
        finally:
            if not on_handle:
                handle.close()
    else:
        if on_handle:
            def score_of(i0, i1):
                return ann.score_matrix(X, cols, i0, i1, which)
        elif hasattr(X, "tocsr"):
            Xm = X.tocsc()[:, cols].tocsr()
            def score_of(i0, i1):
                return ann.score(np.ascontiguousarray(Xm[i0:i1].toarray(), dtype=np.float32))
        else:
            Xd = np.asarray(X)
            def score_of(i0, i1):
                return ann.score(np.ascontiguousarray(Xd[i0:i1][:, cols], dtype=np.float32))
        with Annotator(*ref_args, device=device) as ann:
            out = _run(ann, score_of, n, chunk, fine_tune, False)
    if not fine_tune:
        out["labels"] = out["first_labels"].copy()
        out["tuned_best"], out["tuned_next"] = _best_two(out["scores"])
        out["iterations"] = np.zeros(rows, dtype=np.int32)
    values = np.empty(ref.L, dtype=object)
    values[:] = ref.label_values
    delta, pruned = prune_scores(out["scores"], out["labels"], out["tuned_best"], out["tuned_next"])
    pruned_labels = values[out["labels"]]
    if prune:
        pruned_labels[pruned] = None
    res = {"labels": values[out["labels"]], "first_labels": values[out["first_labels"]], "pruned_labels": pruned_labels,
           "label_ids": out["labels"], "label_values": list(ref.label_values), "scores": out["scores"],
           "tuned_best": out["tuned_best"], "tuned_next": out["tuned_next"], "iterations": out["iterations"], "delta": delta,
           "marker_genes": [names[j] for j in cols], "kernel_ms": out["kernel_ms"]}
    if clusters is not None:
        res.update(cluster_values=cluster_values, cluster_sizes=out["sizes"], cell_labels=res["labels"][cluster_ids])
    return res


def cluster_means(handle, cols, cluster_of, which: str = "normalized"):
    """The rows clusters mode ranks, on their own: ``(means (K, m) float32, sizes (K,) int32)`` of the genes ``cols`` of an
    open ``ExpressionMatrix`` over the cells of each cluster id of ``cluster_of`` (ids in [0, K), K = max + 1, every id
    used).  ``means[c, s] = float32(fp64 sum of x[i, cols[s]] over the cells i of cluster c in ascending order / size)``;
    a sparse handle returns the dense handle's bits.  (:meth:`Annotator.score_clusters` on a one-sample reference.)"""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    of = np.asarray(cluster_of)
    if cols.ndim != 1 or cols.size < 1 or cols.size > MAX_GENES:
        raise ValueError("cols must hold 1 to %d gene indices (got shape %s)" % (MAX_GENES, cols.shape))
    K = int(of.max()) + 1 if of.size else 0
    with Annotator(np.zeros((1, cols.size), dtype=np.float32), np.zeros(1, dtype=np.int32), 1, device=handle.device) as ann:
        sizes = ann.score_clusters(handle, cols, of, K, which)["sizes"]
        return ann.fetch_chunk(), sizes
