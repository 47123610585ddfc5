"""Cluster-quality metrics on the GPU: the numbers the reference publishes for its clusterings.

Reference (R, after the clustering): `/root/reference/R/pbmc3k/Pbmc3k_benchmark_clusters.Rmd`
  :36,47,69  within-cluster average Jaccard distance   ``mean(proxy::dist(cells, method = "jaccard"))``
  :82-94     silhouette widths                          ``cluster::silhouette(labels, dist)``
  :98-112    ``fpc::cluster.stats(dist, labels)``        -> ``R/pbmc3k/QA_benchmark.csv`` ...
One all-pairs pass on the device (csrc/metrics_kernels.hip, include/mi_metrics.h) returns per-cell distance
sums per cluster, squared-distance sums, cluster diameters and the separation matrix; every reported number
is a closed form of those, evaluated here in fp64.  No n x n matrix is built unless ``return_distances``.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def _pack_expression_csr(X) -> np.ndarray:
    """:func:`pack_expression` of a ``scipy.sparse`` matrix from its CSR structure, never densified"""
    from . import preprocess
    indptr, indices, data, (n, g) = preprocess.canonical_csr(X)
    W = (g + 63) // 64
    bits = np.zeros((n, W), dtype=np.uint64)
    keep = data != 0                                             # (a stored zero is a zero)
    cols = indices[keep].astype(np.int64)
    word = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))[keep] * W + (cols >> 6)
    if len(word):
        # rows and, inside a row, columns ascend: the entries of one word are adjacent and their bits distinct, so their sum
        # is their union
        first = np.flatnonzero(np.concatenate([[True], word[1:] != word[:-1]]))
        bits.reshape(-1)[word[first]] = np.add.reduceat(np.uint64(1) << (cols & 63).astype(np.uint64), first)
    return bits


def pack_expression(X) -> np.ndarray:
    """(n cells x g genes) -> (n, ceil(g / 64)) uint64 bit rows of the non-zero pattern (bit b of word w =
    gene 64 w + b), the input of the device pass.  ``X``: a dense array, or a ``scipy.sparse`` matrix, which is packed
    from its CSR structure without densifying (a stored zero is a zero)."""
    from . import preprocess                                      # (lazily: preprocess does not import metrics either)
    if preprocess.is_sparse(X):
        return _pack_expression_csr(X)
    B = (np.asarray(X) != 0)
    n, g = B.shape
    W = (g + 63) // 64
    padded = np.zeros((n, W * 64), dtype=bool)
    padded[:, :g] = B
    # little-endian bit order inside bytes, little-endian bytes inside the 64-bit word
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(n, W)


def jaccard_pass(bits: np.ndarray, labels: np.ndarray, K: int, device: int = 0, return_distances: bool = False):
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    n, W = bits.shape
    rowsum = np.empty((n, K))
    sq_all, sq_in = np.empty(n), np.empty(n)
    diam, sep = np.empty(K), np.empty((K, K))
    D = np.empty((n, n), dtype=np.float32) if return_distances else None
    ms = _lib.call_ms("mi_jaccard_cluster_stats", bits, n, W, labels, int(K), int(device), rowsum, sq_all, sq_in, diam, sep, D)
    return {"rowsum": rowsum, "sq_all": sq_all, "sq_within": sq_in, "diameter": diam, "separation.matrix": sep,
            "distances": D, "kernel_ms": ms}


def cluster_stats(X, labels, device: int = 0, return_distances: bool = False) -> dict:
    """``X``: cells x genes expression (any dtype; only the zero / non-zero pattern enters the binary Jaccard
    distance), dense or ``scipy.sparse`` (e.g. ``fetch_normalized()`` of a sparse handle), or pre-packed uint64 bit rows;
    ``labels``: one non-negative cluster id per cell.  Returns the
    distance-based fields of ``fpc::cluster.stats`` under fpc's names, ``sil.widths`` (``cluster::silhouette``)
    and ``within.average.distance`` (the per-cluster mean the notebook computes at :36)."""
    from . import preprocess
    if preprocess.is_sparse(X):
        bits = pack_expression(X)
    else:
        X = np.asarray(X)
        bits = X if X.dtype == np.uint64 else pack_expression(X)
    labels = np.asarray(labels)
    if labels.ndim != 1 or len(labels) != bits.shape[0]:
        raise ValueError("labels must have one entry per cell")
    uniq, lab = np.unique(labels, return_inverse=True)             # cluster ids need not be 0..K-1 (random colours)
    K, n = len(uniq), len(lab)
    r = jaccard_pass(bits, lab, K, device, return_distances)
    rs, sizes = r["rowsum"], np.bincount(lab, minlength=K).astype(np.int64)
    own = rs[np.arange(n), lab]
    a = np.where(sizes[lab] > 1, own / np.maximum(sizes[lab] - 1, 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = rs / sizes[None, :]
    means[np.arange(n), lab] = np.inf
    b = means.min(axis=1) if K > 1 else np.zeros(n)
    m = np.maximum(a, b)
    sil = np.where((sizes[lab] > 1) & (K > 1) & (m > 0), (b - a) / np.where(m > 0, m, 1.0), 0.0)
    pair_sum = np.zeros((K, K))                                     # sum of d over ordered pairs (i in c, j in c')
    np.add.at(pair_sum, lab, rs)
    n_within = int((sizes * (sizes - 1) // 2).sum())
    n_between = n * (n - 1) // 2 - n_within
    within_sum = np.trace(pair_sum) / 2.0
    between_sum = (pair_sum.sum() - np.trace(pair_sum)) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        avgd = np.where(sizes > 1, np.diag(pair_sum) / np.maximum(sizes * (sizes - 1), 1), np.nan)
        avbm = pair_sum / (sizes[:, None] * sizes[None, :])
    np.fill_diagonal(avbm, 0.0)
    sepm = r["separation.matrix"]
    off = ~np.eye(K, dtype=bool)
    sep = np.where(off, sepm, np.inf).min(axis=1) if K > 1 else np.full(K, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        toother = (pair_sum.sum(axis=1) - np.diag(pair_sum)) / (sizes * (n - sizes))
    wss = float((np.bincount(lab, weights=r["sq_within"], minlength=K) / 2.0 / np.maximum(sizes, 1)).sum())
    tss = float(r["sq_all"].sum() / 2.0 / n)
    diam = r["diameter"]
    avg_within, avg_between = float(a.sum() / n), (between_sum / n_between if n_between else float("nan"))
    # Pearson correlation of the pair distances with the 0/1 "different clusters" indicator
    npairs = n * (n - 1) // 2
    if n_between and n_within:
        sd, sdd = within_sum + between_sum, float(r["sq_all"].sum() / 2.0)
        cov = between_sum / npairs - (sd / npairs) * (n_between / npairs)
        var_d = sdd / npairs - (sd / npairs) ** 2
        var_i = (n_between / npairs) * (1.0 - n_between / npairs)
        gamma = cov / np.sqrt(var_d * var_i) if var_d > 0 and var_i > 0 else float("nan")
    else:
        gamma = float("nan")
    p = sizes / n
    out = {
        "n": n, "cluster.number": K, "cluster.ids": uniq, "cluster.size": sizes, "min.cluster.size": int(sizes.min()),
        "diameter": diam, "average.distance": avgd, "within.average.distance": avgd, "separation": sep,
        "average.toother": toother, "separation.matrix": sepm, "ave.between.matrix": avbm,
        "average.between": avg_between, "average.within": avg_within, "n.between": int(n_between),
        "n.within": n_within, "max.diameter": float(diam.max()), "min.separation": float(sep.min()),
        "within.cluster.ss": wss,
        "clus.avg.silwidths": np.bincount(lab, weights=sil, minlength=K) / np.maximum(sizes, 1),
        "avg.silwidth": float(sil.mean()), "sil.widths": sil, "pearsongamma": float(gamma),
        "dunn": float(sep.min() / diam.max()) if diam.max() > 0 else float("nan"),
        "dunn2": float(np.nanmin(np.where(off, avbm, np.nan)) / np.nanmax(avgd)) if K > 1 and np.any(sizes > 1) else float("nan"),
        "entropy": float(-(p * np.log(p)).sum()), "wb.ratio": avg_within / avg_between if n_between else float("nan"),
        "ch": ((tss - wss) / (K - 1)) / (wss / (n - K)) if K > 1 and n > K and wss > 0 else float("nan"),
        "kernel_ms": r["kernel_ms"],
    }
    if return_distances:
        out["distances"] = r["distances"]
    return out


def modularity(G, labels, resolution: float = 1.0) -> float:
    """Weighted modularity ``Q_gamma`` of a labelling (host fp64), what ``networkx.community.modularity(G, communities,
    weight="weight", resolution=gamma)`` returns: ``sum_c [L_c / m - gamma (K_c / 2m)^2]`` with L_c the weight inside
    community c (a self-loop once) and K_c its degree sum (a self-loop twice).  ``labels``: a dict node -> label or a
    sequence in ``G.nodes`` order."""
    nodes = list(G.nodes)
    index = {v: i for i, v in enumerate(nodes)}
    lab = np.asarray([labels[v] for v in nodes] if isinstance(labels, dict) else labels).reshape(-1)
    if len(lab) != len(nodes):
        raise ValueError("labels must cover every node of G")
    _, lab = np.unique(lab, return_inverse=True)
    eu, ev, w = [], [], []
    for u, v, d in G.edges(data="weight", default=1):
        eu.append(index[u])
        ev.append(index[v])
        w.append(float(d))
    eu, ev, w = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64), np.asarray(w, dtype=np.float64)
    k = np.zeros(len(nodes))
    np.add.at(k, eu, w)
    np.add.at(k, ev, w)
    m = float(np.sum(k)) / 2.0
    if m <= 0.0:
        raise ValueError("modularity is undefined on a graph without edges")
    inside = float(np.sum(w[lab[eu] == lab[ev]]))
    Kc = np.bincount(lab, weights=k)
    return inside / m - float(resolution) * float(np.sum((Kc / (2.0 * m)) ** 2))


# ---------------------------------------------------------------------------------------------------------------------
# Label agreement: adjusted Rand index and normalised mutual information between labellings (include/mi_metrics.h
# mi_label_agreement_u16, csrc/agreement_kernels.hip).  The contingency table of every pair is an exact integer product
# on the i8 matrix cores; ARI (Hubert-Arabie) and NMI (arithmetic) are evaluated from it in fp64 on the device, with
# sklearn's conventions for the degenerate cases.
# ---------------------------------------------------------------------------------------------------------------------
AGREE_CROSS, AGREE_WITHIN = 0, 1
MAX_AGREE_LABELS = 64


def _labellings(L, name: str):
    """(n,) or (R, n) labels -> (R, n) uint16 in [0, K) and K.  A labelling with a label outside [0, 64) is compacted
    (its distinct labels renumbered in sorted order); more than 64 distinct labels raise ValueError."""
    A = np.asarray(L)
    if A.ndim == 1:
        A = A[None, :]
    if A.ndim != 2:
        raise ValueError("%s must be (n,) or (R, n) labels (got shape %s)" % (name, np.shape(L)))
    if A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("%s needs at least one labelling of at least one cell (got shape %s)" % (name, A.shape))
    if np.issubdtype(A.dtype, np.integer) and A.min() >= 0 and A.max() < MAX_AGREE_LABELS:
        out = A.astype(np.uint16)
    else:
        out = np.empty(A.shape, dtype=np.uint16)
        for r in range(A.shape[0]):
            row = A[r]
            if np.issubdtype(row.dtype, np.integer) and row.min() >= 0 and row.max() < MAX_AGREE_LABELS:
                out[r] = row
                continue
            uniq, inv = np.unique(row, return_inverse=True)
            if len(uniq) > MAX_AGREE_LABELS:
                raise ValueError("%s: labelling %d has %d distinct labels (at most %d)" % (name, r, len(uniq), MAX_AGREE_LABELS))
            out[r] = inv.reshape(-1)
    return np.ascontiguousarray(out), int(out.max()) + 1


def label_agreement(A, B=None, groups: int = 1, device: int = 0, tables: bool = False) -> dict:
    """All pairs of labellings at once.  ``B`` given: every (row of A, row of B) pair, arrays of shape (Ra, Rb).  ``B``
    None: every pair r < s inside each of ``groups`` groups of consecutive rows of A, flat in row-major order, group
    after group.  Returns ``ari``, ``nmi``, ``pair_sum`` (sum of C(n_ij, 2), int64), ``tables`` (B given and
    ``tables``: (Ra, Rb, Ka, Kb) int32 contingency tables; else None) and ``kernel_ms``."""
    La, Ka = _labellings(A, "A")
    Ra, n = La.shape
    if B is not None:
        Lb, Kb = _labellings(B, "B")
        Rb = Lb.shape[0]
        if Lb.shape[1] != n:
            raise ValueError("A and B label different numbers of cells (%d, %d)" % (n, Lb.shape[1]))
        if int(groups) != 1:
            raise ValueError("groups apply to the pairs within A only")
        shape, mode = (Ra, Rb), AGREE_CROSS
    else:
        Lb, Kb, Rb = None, Ka, 0
        G = int(groups)
        if G < 1 or Ra % G:
            raise ValueError("%d labellings do not split into %d equal groups" % (Ra, G))
        Rg = Ra // G
        shape, mode = (G * Rg * (Rg - 1) // 2,), AGREE_WITHIN
        if tables:
            raise ValueError("contingency tables are returned for pairs across A and B only")
    ari, nmi = np.empty(shape), np.empty(shape)
    S = np.empty(shape, dtype=np.int64)
    T = np.empty(shape + (Ka, Kb), dtype=np.int32) if tables else None
    ms = _lib.call_ms("mi_label_agreement_u16", La, Ra, Lb, Rb, n, Ka, Kb, mode, int(groups), int(device), ari, nmi, S, T)
    return {"ari": ari, "nmi": nmi, "pair_sum": S, "tables": T, "kernel_ms": ms}


def _against(a, b, key: str, device: int):
    A = np.asarray(a)
    if np.ndim(b) != 1:
        raise ValueError("b must be one labelling of shape (n,)")
    r = label_agreement(A, b, device=device)[key][:, 0]
    return float(r[0]) if A.ndim == 1 else r


def adjusted_rand_index(a, b, device: int = 0):
    """ARI of labelling ``a`` (n,) against ``b`` (n,), a float; or of every row of ``a`` (R, n), an (R,) array."""
    return _against(a, b, "ari", device)


def normalized_mutual_info(a, b, device: int = 0):
    """NMI (arithmetic normalisation) of ``a`` (n,) or every row of ``a`` (R, n) against ``b`` (n,)."""
    return _against(a, b, "nmi", device)


def contingency(a, b, device: int = 0) -> np.ndarray:
    """The exact contingency table of two labellings (n,): entry (i, j) counts the cells labelled i by ``a`` and j by
    ``b``; rows 0 .. max(a), columns 0 .. max(b) (after compaction of labels outside [0, 64))."""
    if np.ndim(a) != 1 or np.ndim(b) != 1:
        raise ValueError("contingency takes two labellings of shape (n,)")
    return label_agreement(a, b, device=device, tables=True)["tables"][0, 0].astype(np.int64)


def pairwise_agreement(L, other=None, groups: int = 1, device: int = 0):
    """ARI and NMI matrices.  ``other`` given: (Ra, Rb) between the rows of ``L`` and of ``other``.  Else the rows of
    ``L`` against each other: (R, R), symmetric with a diagonal of 1; with ``groups`` > 1 only pairs inside each group
    of R / groups consecutive rows, as (groups, R / groups, R / groups)."""
    if other is not None:
        r = label_agreement(L, other, groups=groups, device=device)
        return r["ari"], r["nmi"]
    r = label_agreement(L, None, groups=groups, device=device)
    R = np.asarray(L).shape[0] if np.ndim(L) == 2 else 1
    G = int(groups)
    Rg = R // G
    iu = np.triu_indices(Rg, 1)
    out = []
    for key in ("ari", "nmi"):
        M = np.zeros((G, Rg, Rg))
        flat = r[key].reshape(G, -1)
        for g in range(G):
            M[g][iu] = flat[g]
            M[g] = M[g] + M[g].T
            np.fill_diagonal(M[g], 1.0)
        out.append(M[0] if G == 1 else M)
    return out[0], out[1]


def mean_pair_agreement(ari, nmi):
    """(mean ARI, mean NMI) over a flat array of pairs in a fixed-order fp64 sum (math.fsum); None with no pair."""
    import math
    if len(ari) == 0:
        return None, None
    return math.fsum(ari) / len(ari), math.fsum(nmi) / len(nmi)


def replica_stability(sampleset, device: int = 0):
    """Mean pairwise ARI over the READS of a sampleset: aggregated records are expanded by ``num_occurrences`` (two
    reads of one record agree with ARI 1).  None with fewer than two reads."""
    rec = sampleset.record
    L = np.repeat(np.asarray(rec["sample"]), np.asarray(rec["num_occurrences"], dtype=np.int64), axis=0)
    if L.shape[0] < 2:
        return None
    r = label_agreement(L, None, device=device)
    return mean_pair_agreement(r["ari"], r["nmi"])[0]


# ---------------------------------------------------------------------------------------------------------------------
# Consensus of a set of labellings ("reads"): the co-association matrix C[i, j] = number of reads that put cells i and j
# in one cluster (Monti et al. 2003; Fred and Jain 2005), its distribution (consensus CDF, PAC of Senbabaoglu et al.
# 2014), a per-cell confidence, and the consensus partition of Lancichinetti and Fortunato 2012 restricted to a graph's
# edges.  include/mi_metrics.h mi_coassociation_u16, csrc/coassoc_kernels.hip: the matrix is an exact integer product on
# the i8 matrix cores that is reduced tile by tile and never stored unless asked for.
# ---------------------------------------------------------------------------------------------------------------------
def _edge_arrays(edges, n: int):
    """``edges``: (eu, ev) or an (m, 2) array of cell indices -> two contiguous int32 arrays, checked against [0, n)."""
    if isinstance(edges, tuple) and len(edges) == 2:
        eu, ev = np.asarray(edges[0]), np.asarray(edges[1])
    else:
        E = np.asarray(edges)
        if E.ndim != 2 or E.shape[1] != 2:
            raise ValueError("edges must be (eu, ev) or an (m, 2) array")
        eu, ev = E[:, 0], E[:, 1]
    if eu.shape != ev.shape or eu.ndim != 1:
        raise ValueError("eu and ev must be two 1-D arrays of one length")
    if len(eu) and (min(eu.min(), ev.min()) < 0 or max(eu.max(), ev.max()) >= n):
        raise ValueError("edge index outside [0, %d)" % n)
    return np.ascontiguousarray(eu, dtype=np.int32), np.ascontiguousarray(ev, dtype=np.int32)


def _coassoc_outputs(G: int, Rg: int, n: int, Kref, m, matrix: bool, hist: bool = True):
    hist = np.zeros((G, Rg + 1), dtype=np.int64) if hist else None
    rowsum = np.zeros((G, n, Kref), dtype=np.int64) if Kref is not None else None
    edge = np.zeros((G, m), dtype=np.int32) if m is not None else None
    counts = np.zeros((G, n, n), dtype=np.int32) if matrix else None
    return hist, rowsum, edge, counts


def _coassoc_result(G, Rg, hist, rowsum, edge, counts, ms):
    one = G == 1
    pick = (lambda a: None if a is None else (a[0] if one else a))
    return {"hist": pick(hist), "rowsum": pick(rowsum), "edge_counts": pick(edge), "counts": pick(counts),
            "reads_per_group": Rg, "kernel_ms": float(ms)}


def coassociation(L, groups: int = 1, ref=None, edges=None, matrix: bool = False, device: int = 0,
                  hist: bool = True) -> dict:
    """Co-association of the rows of ``L`` ((R, n) labels) inside each of ``groups`` groups of R / groups consecutive
    rows: ``C[i, j]`` = number of rows of the group with ``L[r, i] == L[r, j]``.  Returns
      ``hist``         (Rg + 1,) int64: number of pairs i < j with C[i, j] == v (None with ``hist=False``; with only
                       ``edges`` besides, the dense pass is then skipped and nothing depends on n x n: any n)
      ``rowsum``       (n, Kref) int64, only with ``ref`` ((n,) or (groups, n) reference labels): sum of C[i, j] over
                       j != i with ref[j] == c
      ``edge_counts``  (m,) int32, only with ``edges`` ((eu, ev) or (m, 2)): C[eu, ev]
      ``counts``       (n, n) int32, only with ``matrix``
      ``reads_per_group`` and ``kernel_ms``;
    with ``groups`` > 1 every array has a leading axis of that length.  Labels outside [0, 64) are compacted per
    labelling as in :func:`label_agreement`."""
    La, K = _labellings(L, "L")
    R, n = La.shape
    G = int(groups)
    if G < 1 or R % G:
        raise ValueError("%d labellings do not split into %d equal groups" % (R, G))
    Rg = R // G
    Lr, Kref = None, None
    if ref is not None:
        Lr, Kref = _labellings(ref, "ref")
        if Lr.shape[1] != n:
            raise ValueError("ref labels %d cells, L labels %d" % (Lr.shape[1], n))
        if Lr.shape[0] == 1 and G > 1:
            Lr = np.ascontiguousarray(np.repeat(Lr, G, axis=0))
        if Lr.shape[0] != G:
            raise ValueError("ref must be (n,) or (groups, n)")
    eu = ev = None
    if edges is not None:
        eu, ev = _edge_arrays(edges, n)
    hist, rowsum, edge, counts = _coassoc_outputs(G, Rg, n, Kref, None if eu is None else len(eu), matrix, hist)
    ms = _lib.call_ms("mi_coassociation_u16", La, R, n, K, G, Lr, int(Kref or 1), eu, ev, 0 if eu is None else len(eu),
                      int(device), hist, rowsum, edge, counts)
    return _coassoc_result(G, Rg, hist, rowsum, edge, counts, ms)


def consensus_cdf(hist) -> np.ndarray:
    """Empirical CDF of the consensus index C / Rg over the pairs: entry v = share of pairs with C <= v (v = 0 .. Rg;
    the last axis of ``hist``).  All zeros where there is no pair."""
    h = np.asarray(hist, dtype=np.float64)
    tot = h.sum(axis=-1, keepdims=True)
    return np.cumsum(h, axis=-1) / np.where(tot > 0, tot, 1.0)


def pac(hist, lo: float = 0.1, hi: float = 0.9):
    """Proportion of ambiguous clustering: the share of pairs with ``lo < C / Rg < hi`` (strict on both sides, compared
    as integers against ``lo * Rg`` and ``hi * Rg``).  0.0 where there is no pair.  A float, or an array over the
    leading axes of ``hist``."""
    h = np.asarray(hist, dtype=np.int64)
    Rg = h.shape[-1] - 1
    v = np.arange(Rg + 1, dtype=np.float64)
    amb = (v > lo * Rg) & (v < hi * Rg)
    tot = h.sum(axis=-1)
    out = (h * amb).sum(axis=-1) / np.where(tot > 0, tot, 1)
    return float(out) if np.ndim(out) == 0 else out


def cell_confidence(rowsum, ref, reads: int) -> np.ndarray:
    """Per cell i the mean consensus index with the other members of its own cluster of ``ref``:
    ``rowsum[i, ref_i] / (reads * (|cluster(ref_i)| - 1))``; 1.0 for a singleton.  ``ref`` as given to
    :func:`coassociation` (its labels compacted the same way when outside [0, 64))."""
    lab = _labellings(ref, "ref")[0][0].astype(np.int64)
    rs = np.asarray(rowsum)
    if rs.ndim != 2 or rs.shape[0] != len(lab):
        raise ValueError("rowsum must be (n, Kref) for the n cells of ref")
    sizes = np.bincount(lab, minlength=rs.shape[1])
    own = rs[np.arange(len(lab)), lab].astype(np.float64)
    den = float(reads) * (sizes[lab] - 1)
    return np.where(sizes[lab] > 1, own / np.where(den > 0, den, 1.0), 1.0)


def consensus_labels(edge_counts, reads: int, eu, ev, n: int, tau: float = 0.5) -> np.ndarray:
    """Connected components of the edges with ``edge_counts >= tau * reads`` over cells 0 .. n - 1 (host union-find),
    numbered by their smallest cell in ascending order: the partition the Lancichinetti-Fortunato consensus loop ends in
    when it converges; before that Fred and Jain's single-link cut at ``tau`` restricted to the graph."""
    ec, eu, ev = np.asarray(edge_counts), np.asarray(eu), np.asarray(ev)
    if not (ec.shape == eu.shape == ev.shape) or ec.ndim != 1:
        raise ValueError("edge_counts, eu and ev must be three 1-D arrays of one length")
    keep = ec >= tau * reads
    parent = list(range(int(n)))
    for a, b in zip(eu[keep].tolist(), ev[keep].tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:                                   # the smaller cell is the root: a root is its component's minimum
            if a < b:
                parent[b] = a
            else:
                parent[a] = b
    root = np.empty(int(n), dtype=np.int64)
    for i in range(int(n)):
        root[i] = i if parent[i] == i else root[parent[i]]          # parent[i] < i for every non-root
    return np.unique(root, return_inverse=True)[1].reshape(-1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Connected components of one graph under a per-item edge filter, many items at once (include/mi_metrics.h
# mi_graph_components, csrc/components_kernels.hip): a labelling's "same label" filter splits its clusters into their
# connected pieces -- the guarantee of Leiden's refinement step (Traag et al. 2019), not Leiden itself -- and a mask over
# the edges gives the consensus partition of :func:`consensus_labels` for every resolution group in one call.
# ---------------------------------------------------------------------------------------------------------------------
COMPONENTS_LDS_MAX_CELLS = 26624           # MI_COMPONENTS_LDS_MAX_CELLS (include/mi_metrics.h)


def _graph_csr(edges_or_csr, n: int):
    """``(rowptr, col)`` (len n + 1 with rowptr[-1] == len(col)) or edges ((eu, ev) / (m, 2)) -> ``(rowptr, col, order)``:
    int32 CSR and, for edges, the position of every stored entry in the caller's edge list (each edge is stored once,
    under its first end; None for a CSR)."""
    n = int(n)
    if isinstance(edges_or_csr, tuple) and len(edges_or_csr) == 2:
        a, b = np.asarray(edges_or_csr[0]), np.asarray(edges_or_csr[1])
        if a.ndim == 1 and b.ndim == 1 and len(a) == n + 1 and int(a[-1]) == len(b):      # (an edge index is < n <= len(b) - 1)
            return np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32), None
    eu, ev = _edge_arrays(edges_or_csr, n)
    order = np.argsort(eu, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(eu, minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), np.ascontiguousarray(ev[order]), order


def _labels_u16(labels, n: int):
    """(n,) or (B, n) labels -> (B, n) uint16.  Labels outside [0, 65536) are compacted per labelling (distinct labels
    renumbered in sorted order), as :func:`_labellings` does for its narrower range."""
    A = np.asarray(labels)
    if A.ndim == 1:
        A = A[None, :]
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != n:
        raise ValueError("labels must be (n,) or (B, n) with n = %d (got shape %s)" % (n, np.shape(labels)))
    if np.issubdtype(A.dtype, np.integer) and A.min() >= 0 and A.max() < 65536:
        return np.ascontiguousarray(A, dtype=np.uint16)
    out = np.empty(A.shape, dtype=np.uint16)
    for r in range(A.shape[0]):
        uniq, inv = np.unique(A[r], return_inverse=True)
        if len(uniq) > 65536:
            raise ValueError("labelling %d has %d distinct labels (at most 65536)" % (r, len(uniq)))
        out[r] = inv.reshape(-1)
    return out


def connected_components(edges_or_csr, n: int, labels=None, keep=None, device: int = 0, force_global: bool = False):
    """Connected components of the graph on cells 0 .. n - 1 for a batch of B items.  ``edges_or_csr``: ``(eu, ev)`` /
    an (m, 2) array (every edge once is enough) or ``(rowptr, col)``.  ``labels`` ((n,) = one item, or (B, n)): item b
    keeps the edges whose ends carry one label.  ``keep`` ((B, m) or (m,) over the edges, or over the CSR entries):
    item b keeps the entries with ``keep[b, e] != 0``; an edge stored in both directions connects when either is kept.
    With neither, B = 1.  Self loops connect nothing.  Returns ``(labels int32 (B, n), counts int32 (B,))``: components
    numbered 0 .. C_b - 1 by their smallest cell, ascending (the numbering of :func:`consensus_labels`).
    ``force_global``: the kernel's global form (parent array in HBM), which otherwise serves n >
    ``COMPONENTS_LDS_MAX_CELLS``."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1 (got %d)" % n)
    rowptr, col, order = _graph_csr(edges_or_csr, n)
    nnz = len(col)
    L = None if labels is None else _labels_u16(labels, n)
    K = None
    if keep is not None:
        K = np.asarray(keep)
        if K.ndim == 1:
            K = K[None, :]
        if K.ndim != 2 or K.shape[1] != nnz:
            raise ValueError("keep must be (m,) or (B, m) over the %d edges (got shape %s)" % (nnz, np.shape(keep)))
        K = K != 0
        if order is not None:
            K = K[:, order]
        K = np.ascontiguousarray(K, dtype=np.uint8)
    if L is not None and K is not None and L.shape[0] != K.shape[0]:
        raise ValueError("labels give %d items, keep gives %d" % (L.shape[0], K.shape[0]))
    B = L.shape[0] if L is not None else (K.shape[0] if K is not None else 1)
    out = np.empty((B, n), dtype=np.int32)
    cnt = np.empty(B, dtype=np.int32)
    _lib.call("mi_graph_components", rowptr, col, n, L, K, int(B), int(device), 1 if force_global else 0, out, cnt, None)
    return out, cnt


def split_disconnected(edges_or_csr, n: int, labels, device: int = 0):
    """Every cluster of every labelling split into its connected components in the graph: ``(refined labels int32 (B, n),
    cluster counts (B,))``, numbered by smallest cell as :func:`connected_components`.  A refined cluster lies inside one
    original cluster and is connected; a labelling whose clusters are all connected keeps its partition."""
    return connected_components(edges_or_csr, n, labels=labels, device=device)


def renumber_by_first_cell(labels) -> np.ndarray:
    """(B, n) non-negative labels -> the same partitions numbered 0, 1, ... in the order their first cell appears."""
    A = np.asarray(labels)
    B, n = A.shape
    width = int(A.max()) + 1
    flat = (np.arange(B, dtype=np.int64)[:, None] * width + A).reshape(-1)
    uniq, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")              # (a flat position grows with the item, then with the cell)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    start = np.searchsorted(first[order] // n, np.arange(B))         # rank of every item's first cluster
    return (rank[inv.reshape(-1)].reshape(B, n) - start[:, None]).astype(np.int32)


def confidence_passes(labels):
    """The reference labellings :func:`cell_confidence_any` needs for ``labels``: per pass ``(ref, inside)``, 63 clusters in
    order of decreasing size (ties: the smaller label first) under labels 0 .. 62 with every other cell under label 63;
    ``inside`` marks the cells whose confidence the pass gives.  Singletons (confidence 1.0) need no pass."""
    uniq, lab = np.unique(np.asarray(labels), return_inverse=True)
    lab = lab.reshape(-1)
    sizes = np.bincount(lab, minlength=len(uniq))
    order = np.argsort(-sizes, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    out = []
    for lo in range(0, int((sizes > 1).sum()), 63):
        rk = rank[lab] - lo
        inside = (rk >= 0) & (rk < 63)
        out.append((np.where(inside, rk, 63).astype(np.int64), inside))
    return out


def cell_confidence_any(rowsum_fn, labels, reads: int) -> np.ndarray:
    """:func:`cell_confidence` for a labelling with any number of clusters.  ``rowsum_fn(ref)`` returns the (n, Kref) row
    sums for reference labels in [0, 64); one call per pass of :func:`confidence_passes`."""
    conf = np.ones(len(np.asarray(labels).reshape(-1)))
    for ref, inside in confidence_passes(labels):
        c = cell_confidence(np.asarray(rowsum_fn(ref)), ref, reads)
        conf[inside] = c[inside]
    return conf


# ---------------------------------------------------------------------------------------------------------------------
# Marker genes: the Wilcoxon rank-sum test of every cluster against all other cells, per gene (Seurat's FindAllMarkers with
# its default test), for many labellings in one device call (include/mi_metrics.h mi_rank_sum_markers_f32 on a host array,
# include/mi_prep.h mi_prep_rank_sum_markers on a resident ExpressionMatrix, dense or sparse; csrc/markers_kernels.hip).  A gene's ranks do not depend on the labelling: the device sorts every gene once and returns
# exact integer rank sums, counts and the tie term; everything reported is a closed form of those, evaluated here in fp64.
# ---------------------------------------------------------------------------------------------------------------------
MARKERS_LDS_MAX_NONZEROS = 8192            # MI_MARKERS_LDS_MAX_NONZEROS (include/mi_metrics.h)
MARKERS_LABELLING_CHUNK = 16               # MI_MARKERS_LABELLING_CHUNK
MARKERS_SUM_PLAIN, MARKERS_GLOBAL = 1, 2

try:
    from scipy.special import erfc as _erfc
except ImportError:                        # the package does not need scipy
    import math
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _resident(X, which):
    """``(handle, which, owned)`` for an ``X`` that is ranked on the device where it lies -- an open
    :class:`preprocess.ExpressionMatrix`, or a ``scipy.sparse`` matrix, which is uploaded through a temporary handle as the
    values to rank -- and ``None`` for a dense array.  ``which`` of a handle defaults to ``"normalized"`` once it has been
    normalised, else ``"counts"``.  The errors are raised before any library call."""
    from . import preprocess                                      # (lazily: preprocess does not import metrics either)
    if isinstance(X, preprocess.ExpressionMatrix):
        if which is None:
            which = "normalized" if X.normalized else "counts"
        if which not in ("counts", "normalized"):
            raise ValueError("which must be 'counts' or 'normalized'")
        X._handle()                                               # ValueError for a closed handle
        return X, which, False
    if preprocess.is_sparse(X):
        if which not in (None, "counts"):
            raise ValueError("a sparse matrix holds the values to rank: which must be 'counts' (or None)")
        if X.ndim != 2:
            raise ValueError("X must be (cells, genes) (got shape %s)" % (X.shape,))
        return None, "counts", True
    if which is not None:
        raise TypeError("which= applies to an ExpressionMatrix or a scipy.sparse matrix, not to a dense array")
    return None


def _check_labels_shape(L, n):
    L = np.asarray(L)
    if L.ndim == 1:
        L = L[None, :]
    if L.ndim != 2 or L.shape[1] != n:
        raise ValueError("X must be (n, g) and L (n,) or (B, n) (got n = %d, %s)" % (n, L.shape))
    return L


def rank_sum_pass(X, L, K: int, device: int = 0, plain: bool = False, force_global: bool = False, which=None) -> dict:
    """The device pass.  ``X``: cells x genes, finite; ``L``: (n,) or (B, n) labels in [0, K), K <= 64.  ``X`` may also be
    an open :class:`preprocess.ExpressionMatrix` (``which``: its ``"counts"`` or ``"normalized"`` matrix, by default the
    normalised one once it exists; ranked where it lies, ``device`` is the handle's) or a ``scipy.sparse`` matrix of the
    values to rank, which must be non-negative (uploaded as CSR, never densified); both give the bits of the dense array.
    Returns, per
    (labelling, gene, cluster), ``rank2`` (int64, twice the sum of the cluster's midranks among all n cells), ``npos``
    (int32, its cells with x > 0) and ``sum`` (fp64, the sum of ``expm1(x)`` over its cells in cell order; of ``x`` with
    ``plain``); ``tie`` (g,) int64, the sum of t^3 - t over each gene's tie groups; and ``kernel_ms``.
    ``force_global``: the ranking kernel's HBM form, which otherwise serves genes with more than
    ``MARKERS_LDS_MAX_NONZEROS`` non-zero cells."""
    res = _resident(X, which)
    if res is not None:
        handle, which, owned = res
        L = _check_labels_shape(L, X.n if handle is not None else X.shape[0])
        if not owned:
            return handle.rank_sum_pass(L, K, which=which, plain=plain, force_global=force_global)
        from . import preprocess
        with preprocess.ExpressionMatrix(X, device=device) as m:
            return m.rank_sum_pass(L, K, which="counts", plain=plain, force_global=force_global)
    X = np.ascontiguousarray(X, dtype=np.float32)
    L = np.asarray(L)
    if L.ndim == 1:
        L = L[None, :]
    if X.ndim != 2 or L.ndim != 2 or L.shape[1] != X.shape[0]:
        raise ValueError("X must be (n, g) and L (n,) or (B, n) (got %s, %s)" % (X.shape, L.shape))
    if L.size and (L.min() < 0 or L.max() > 65535):
        raise ValueError("labels must lie in [0, K)")
    L = np.ascontiguousarray(L, dtype=np.uint16)
    (n, g), B, K = X.shape, L.shape[0], int(K)
    shape = (B, g, max(K, 0))
    rank2, npos = np.empty(shape, dtype=np.int64), np.empty(shape, dtype=np.int32)
    sums, tie = np.empty(shape, dtype=np.float64), np.empty(g, dtype=np.int64)
    ms = _lib.call_ms("mi_rank_sum_markers_f32", X, n, g, L, B, K, int(device),
                      (MARKERS_SUM_PLAIN if plain else 0) | (MARKERS_GLOBAL if force_global else 0), rank2, npos, sums, tie)
    return {"rank2": rank2, "npos": npos, "sum": sums, "tie": tie, "kernel_ms": ms}


def markers_from_stats(rank2, npos, sums, tie, sizes, n: int, plain: bool = False) -> dict:
    """Host fp64 closed forms of the rank-sum statistics.  ``rank2``, ``npos``, ``sums``: (..., g, K); ``tie``: (g,);
    ``sizes``: (..., K) cluster sizes; ``n`` cells.  With n1 the cluster's size and n2 = n - n1, per (..., gene, cluster):
      ``U``           rank2 / 2 - n1 (n1 + 1) / 2, the Mann-Whitney statistic of the cluster
      ``p_val``       min(1, erfc(z / sqrt 2)), z = (|U - n1 n2 / 2| - 0.5) / sigma, sigma^2 = n1 n2 / 12 ((n + 1) - tie /
                      (n (n - 1))): the two-sided normal approximation with tie and continuity corrections (R's
                      ``wilcox.test(exact = FALSE, correct = TRUE)``, scipy's asymptotic ``mannwhitneyu``); NaN where n1 = 0,
                      n2 = 0 or sigma = 0
      ``p_val_adj``   min(1, p_val * g) (Bonferroni over all genes)
      ``pct_1``, ``pct_2``  share of the cluster's / the other cells with x > 0
      ``avg_log2FC``  log2(mean1 + 1) - log2(mean2 + 1), the means of ``sums`` inside and outside the cluster
      ``auc``         U / (n1 n2)
    and with ``plain`` (``sums`` of scaled data) also ``avg_diff`` = mean1 - mean2."""
    rank2, npos, sums = np.asarray(rank2, dtype=np.float64), np.asarray(npos, dtype=np.float64), np.asarray(sums, dtype=np.float64)
    g = rank2.shape[-2]
    n = int(n)
    n1 = np.asarray(sizes, dtype=np.float64)[..., None, :]
    n2 = n - n1
    tie = np.asarray(tie, dtype=np.float64).reshape(g, 1)
    U = rank2 / 2.0 - n1 * (n1 + 1.0) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        var = n1 * n2 / 12.0 * ((n + 1.0) - tie / (n * (n - 1.0))) if n > 1 else np.zeros_like(U)
        sigma = np.sqrt(np.maximum(var, 0.0))
        ok = (n1 > 0) & (n2 > 0) & (sigma > 0)
        z = (np.abs(U - n1 * n2 / 2.0) - 0.5) / np.where(ok, sigma, 1.0)
        p = np.where(ok, np.minimum(1.0, _erfc(z / np.sqrt(2.0))), np.nan)
        pct1 = np.where(n1 > 0, npos / n1, np.nan)
        pct2 = np.where(n2 > 0, (npos.sum(axis=-1, keepdims=True) - npos) / n2, np.nan)
        mean1 = np.where(n1 > 0, sums / n1, np.nan)
        mean2 = np.where(n2 > 0, (sums.sum(axis=-1, keepdims=True) - sums) / n2, np.nan)
        out = {"U": U, "p_val": p, "p_val_adj": np.minimum(1.0, p * g), "pct_1": pct1, "pct_2": pct2,
               "avg_log2FC": np.log2(mean1 + 1.0) - np.log2(mean2 + 1.0),
               "auc": np.where((n1 > 0) & (n2 > 0), U / np.where(n1 * n2 > 0, n1 * n2, 1.0), np.nan)}
    if plain:
        out["avg_diff"] = mean1 - mean2
    return out


def markers_passed(stats: dict, only_pos: bool = False, min_pct: float = 0.1, logfc_threshold: float = 0.25) -> np.ndarray:
    """Seurat's filter on the fields of :func:`markers_from_stats`: ``max(round(pct_1, 3), round(pct_2, 3)) >= min_pct`` and
    ``avg_log2FC >= logfc_threshold`` (``only_pos``) or ``|avg_log2FC| >= logfc_threshold``.  False where undefined."""
    fc = stats["avg_log2FC"]
    with np.errstate(invalid="ignore"):
        pct = np.fmax(np.round(stats["pct_1"], 3), np.round(stats["pct_2"], 3)) >= min_pct
        return pct & ((fc if only_pos else np.abs(fc)) >= logfc_threshold)


def find_all_markers(X, labels, only_pos: bool = False, min_pct: float = 0.1, logfc_threshold: float = 0.25, genes=None,
                     device: int = 0, plain: bool = False, which=None) -> dict:
    """Seurat's ``FindAllMarkers`` (Wilcoxon rank-sum, every cluster against all other cells) for one labelling ((n,)) or
    many ((B, n)) in one device call.  ``X``: cells x genes, log-normalised (``plain``: scaled data or counts, whose mean is
    the plain mean): a dense array; an open :class:`preprocess.ExpressionMatrix`, whose resident matrix is ranked without
    an upload (``which``: ``"counts"`` or ``"normalized"``, by default the normalised matrix once the handle has one); or a
    ``scipy.sparse`` matrix of the values to rank, e.g. what ``log_normalize(sparse)`` returns -- its values must be
    non-negative, it is uploaded as CSR and no n x g buffer is made.  All three give the same bits.
    Cluster ids are any values, at most 64 distinct over all labellings.  Returns the fields of
    :func:`markers_from_stats`, shaped (g, K) or (B, g, K), ``passed`` (:func:`markers_passed`), ``cluster_ids`` (K,),
    ``cluster_size`` ((K,) or (B, K); a labelling that does not use an id has size 0 and NaN statistics there),
    ``genes`` (the names, default 0 .. g - 1) and ``kernel_ms``."""
    res = _resident(X, which)
    if res is None:
        X = np.asarray(X)
    lab = np.asarray(labels)
    one = lab.ndim == 1
    shape = (X.n, X.g) if res is not None and res[0] is not None else X.shape
    if lab.ndim not in (1, 2) or len(shape) != 2 or lab.shape[-1] != shape[0]:
        raise ValueError("labels must be (n,) or (B, n) for the n rows of X")
    uniq, inv = np.unique(lab, return_inverse=True)
    if len(uniq) > 64:
        raise ValueError("%d distinct cluster ids (at most 64)" % len(uniq))
    L = inv.reshape((1, -1) if one else lab.shape)
    n, g = (int(v) for v in shape)
    K = len(uniq)
    genes = np.arange(g) if genes is None else np.asarray(genes)
    if genes.shape != (g,):
        raise ValueError("genes must name the %d columns of X" % g)
    sizes = np.stack([np.bincount(row, minlength=K) for row in L]).astype(np.int64)
    r = rank_sum_pass(X, L, K, device=device, plain=plain, which=None if res is None else res[1])
    out = markers_from_stats(r["rank2"], r["npos"], r["sum"], r["tie"], sizes, n, plain=plain)
    out["passed"] = markers_passed(out, only_pos, min_pct, logfc_threshold)
    out["cluster_size"] = sizes
    if one:
        out = {k: v[0] for k, v in out.items()}
    out.update(cluster_ids=uniq, genes=genes, kernel_ms=r["kernel_ms"])
    return out


def top_markers(result: dict, n: int = 2, labelling: int = 0) -> dict:
    """Per cluster id the names of the ``n`` passing genes with the largest ``avg_log2FC`` (ties: the earlier gene), the
    notebook's ``slice_max(n = 2, order_by = avg_log2FC)``; ``labelling`` picks the row of a (B, n) call."""
    fc, ok = np.asarray(result["avg_log2FC"]), np.asarray(result["passed"])
    if fc.ndim == 3:
        fc, ok = fc[labelling], ok[labelling]
    elif labelling != 0:
        raise ValueError("the result holds one labelling")
    out = {}
    for k, cid in enumerate(result["cluster_ids"]):
        idx = np.flatnonzero(ok[:, k])
        order = idx[np.argsort(-fc[idx, k], kind="stable")]
        out[cid.item() if hasattr(cid, "item") else cid] = list(np.asarray(result["genes"])[order[:int(n)]])
    return out


def knn_preservation(nn_high, Y, k=None, device: int = 0) -> float:
    """Mean fraction of each point's high-dimensional neighbours (``nn_high``: n x k_high indices, column 0 the point
    itself, as :func:`umap.knn` and :func:`snn.build_snn` return them; the point itself does not count) found among its
    ``k`` nearest neighbours in the embedding ``Y`` (n x 2 or n x 3; ``k`` counts the point, default ``k_high``).  The
    neighbours in ``Y`` come from the same exact kNN kernel, euclidean."""
    from . import umap
    nn_high = np.asarray(nn_high)
    Y = np.asarray(Y)
    if nn_high.ndim != 2 or nn_high.dtype.kind not in "iu" or nn_high.shape[1] < 2:
        raise ValueError("nn_high must be an (n, k) integer array with k >= 2")
    if Y.ndim != 2 or Y.shape[0] != nn_high.shape[0]:
        raise ValueError("Y must be (n, c) with n = %d" % nn_high.shape[0])
    k = nn_high.shape[1] if k is None else int(k)
    if not 2 <= k <= nn_high.shape[1]:
        raise ValueError("k must lie in [2, %d] (got %d)" % (nn_high.shape[1], k))
    nn_low, _ = umap.knn(Y, k, "euclidean", device)
    hit = (nn_high[:, 1:k, None] == nn_low[:, None, 1:]).any(axis=2)
    return float(hit.mean())
