/*
 * mi_metrics.h -- C ABI of the cluster-quality metrics on MI355X (part of libmi_sa.so).
 *
 * The step immediately AFTER the clustering path: the only numbers the
 * reference publishes come from it.  In the reference it is R:
 *     /root/reference/R/pbmc3k/Pbmc3k_benchmark_clusters.Rmd:36,47,69   mean(proxy::dist(cells, "jaccard")) per cluster
 *     :82-94     cluster::silhouette(labels, proxy::dist(cells, "jaccard"))
 *     :98-112    fpc::cluster.stats(dist, labels)  ->  R/pbmc3k/QA_benchmark.csv, Seurat_benchmark.csv, Kmeans_benchmark.csv
 * mi_jaccard_cluster_stats replaces the O(n^2 g) part of all three: one pass over all pairs of cells that
 * never materialises the n x n distance matrix (unless asked to) and returns the sufficient statistics
 * every one of those numbers is a closed form of (scrna_seq_qannealing_clustering_amd/metrics.py).
 *
 * Distances: binary Jaccard d = 1 - |A & B| / |A | B| on the non-zero pattern of each cell's gene row,
 * evaluated in fp64 (two empty rows: 0).  Conventions as in mi_sa.h.
 *
 * mi_label_agreement_u16 answers "how much do two clusterings agree": the adjusted Rand index (Hubert-Arabie) and the
 * normalised mutual information (arithmetic mean of the entropies) of every pair of labellings, the standard way to
 * pick a resolution from replica stability (mean pairwise ARI of independent runs) or to compare against a reference
 * clustering.  The contingency table of every pair is one integer product of one-hot matrices on the i8 matrix cores
 * (exact: i32 accumulation); mi_sa_problem_label_agreement (mi_sa.h) runs the same on the states a Potts anneal left
 * in HBM.  DESIGN.md section 5c.
 *
 * mi_coassociation_u16 answers "where do the labellings agree": the co-association (consensus) matrix C[i, j] = number of
 * labellings that put cells i and j in one cluster (Monti et al.; Fred and Jain's evidence accumulation), again an exact
 * integer product of one-hot matrices on the i8 matrix cores, now with the cells outside and (labelling, label) inside.
 * The matrix is reduced tile by tile into its histogram (consensus CDF, PAC) and per-cell sums per reference cluster;
 * the entries of a graph's edges come from a second kernel that needs nothing of size n x n.
 *
 * mi_graph_components answers "which cells hang together": the connected components of one shared graph under a per-item
 * edge filter, for many items at once -- a read's "same label" filter (the connected pieces of its clusters, the guarantee
 * of Leiden's refinement step) or a group's "kept by at least half of the reads" mask (the consensus partition).
 * Min-hooking with pointer jumping, the parent array in LDS; mi_sa_problem_components (mi_sa.h) runs the same on the
 * states a Potts anneal left in HBM.  DESIGN.md section 5c.
 *
 * mi_rank_sum_markers_f32 answers "which genes mark a cluster": the sufficient statistics of the Wilcoxon rank-sum test of
 * every cluster against all other cells, per gene, for many labellings at once (Seurat's FindAllMarkers with its default
 * test, the step the reference's assessment notebook runs on the QA labels).  A gene's ranks do not depend on the
 * labelling: every gene is sorted once (its non-zeros only; the zeros are one tie block of known rank) and scored against
 * all labellings.  Rank sums, counts and the tie term are exact integers; the p-value, log fold change and AUC are closed
 * forms of them (metrics.markers_from_stats).  DESIGN.md section 5c.
 */
#ifndef MI_METRICS_H
#define MI_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bits: n x words uint64, bit b of word w of row i = (gene 64 w + b is expressed in cell i); labels in [0, K),
 * K <= 64 (unused labels allowed).  The LDS plan is 64 own rows of (words | 1) words, a tile of 16 rows of `words`
 * words and 192 B, whatever K is: 512 * (words | 1) + 128 * words + 192 bytes <= 160 KB, i.e. words <= 255 (16 320
 * genes); MI_EUNSUPPORTED above that and for K > 64, before anything is launched.  Outputs (host, caller-allocated):
 *   rowsum       n x K   sum over j != i with label c of d(i, j)
 *   rowsq_all    n       sum over j != i of d(i, j)^2
 *   rowsq_within n       the same restricted to j in i's cluster
 *   diameter     K       max d inside cluster c (0 for singletons)
 *   separation   K x K   min d between clusters c, c' (+inf where a cluster is empty; diagonal 0)
 *   out_D        n x n fp32 distance matrix, or NULL (nothing n x n is ever allocated then)
 *   out_kernel_ms        device time of the pass, or NULL */
int mi_jaccard_cluster_stats(const uint64_t *bits, int n, int words, const int32_t *labels, int K, int device,
                             double *rowsum, double *rowsq_all, double *rowsq_within, double *diameter,
                             double *separation, float *out_D, float *out_kernel_ms);

#define MI_AGREE_CROSS  0              /* all Ra x Rb pairs (A row i, B row j), pair index i * Rb + j */
#define MI_AGREE_WITHIN 1              /* all r < s inside each of `groups` groups of Ra / groups consecutive rows of A */
#define MI_AGREE_MAX_LABELLINGS 65536  /* Ra, Rb */
#define MI_AGREE_MAX_TABLE_ENTRIES (1 << 28)   /* Ra * Rb * Ka * Kb when out_tables is given (1 GiB of int32) */

/* A: Ra x n and B: Rb x n uint16 labellings, row-major host arrays, labels in [0, Ka) / [0, Kb), K <= 64 (unused labels
 * allowed).  mode MI_AGREE_CROSS: every (A row, B row) pair, groups = 1.  MI_AGREE_WITHIN: B = NULL (Kb, Rb ignored),
 * every pair r < s inside each group, row-major within a group, group after group (groups x C(Ra / groups, 2) pairs).
 * Outputs (host, caller-allocated, each nullable), per pair:
 *   out_ari       adjusted Rand index; 1.0 when no pair of cells is joined by one labelling and split by the other
 *                 (identical up to renaming, both single-cluster, both all-singletons), as sklearn
 *   out_nmi       normalised mutual information, arithmetic; 1.0 when both labellings have one cluster, 0.0 when exactly
 *                 one does, mutual information clipped at 0 (sklearn's conventions)
 *   out_pair_sum  S = sum over the table of C(n_ij, 2), exact in int64
 *   out_tables    CROSS only: the Ka x Kb contingency table (rows: A's labels) per pair, int32; at most
 *                 MI_AGREE_MAX_TABLE_ENTRIES entries in all (MI_EUNSUPPORTED beyond)
 *   out_kernel_ms device time of the kernels
 * MI_EINVAL for bad shapes, K outside [1, 64], a label >= K, n < 1. */
int mi_label_agreement_u16(const uint16_t *A, int Ra, const uint16_t *B, int Rb, int n, int Ka, int Kb, int mode,
                           int groups, int device, double *out_ari, double *out_nmi, int64_t *out_pair_sum,
                           int32_t *out_tables, float *out_kernel_ms);

#define MI_COASSOC_MAX_READS 8192                  /* R / groups: the workgroup's histogram bins live in LDS (4 B each) */
#define MI_COASSOC_MAX_COUNT_ENTRIES (1 << 28)     /* groups * n * n when out_counts is given (1 GiB of int32) */

/* L: R x n uint16 labellings ("reads"), row-major host array, labels in [0, K), K <= 64 (unused labels allowed); `groups`
 * groups of Rg = R / groups consecutive rows.  C_g[i, j] = #{r in group g : L[r, i] == L[r, j]} (0 <= C <= Rg, C[i, i] = Rg).
 * Outputs (host, caller-allocated, each nullable; the dense pass runs only if one of the first three is given, the edge
 * pass only if out_edge is):
 *   out_hist      groups x (Rg + 1) int64: hist[g][v] = number of pairs i < j with C_g[i, j] == v
 *   out_rowsum    groups x n x Kref int64: sum of C_g[i, j] over j != i with ref[g][j] == c; needs `ref`, groups x n uint16
 *                 reference labels in [0, Kref), Kref <= 64 (ref may be NULL without out_rowsum)
 *   out_edge      groups x m int32: C_g[eu[e], ev[e]] for the m edges (eu, ev in [0, n); any order, repeats allowed),
 *                 computed from the labels for any n (nothing n x n exists)
 *   out_counts    groups x n x n int32, the full symmetric matrix; at most MI_COASSOC_MAX_COUNT_ENTRIES entries in all
 *                 (MI_EUNSUPPORTED beyond).  Without it nothing of size n x n is allocated anywhere.
 *   out_kernel_ms device time of the kernels
 * MI_EINVAL for bad shapes, K or Kref outside [1, 64], R not a multiple of groups, a label >= K (ref: >= Kref), an edge
 * index outside [0, n), out_rowsum without ref.  MI_EUNSUPPORTED, before anything is launched, for Rg >
 * MI_COASSOC_MAX_READS and for out_counts beyond its cap. */
int mi_coassociation_u16(const uint16_t *L, int R, int n, int K, int groups, const uint16_t *ref, int Kref,
                         const int32_t *eu, const int32_t *ev, int64_t m, int device, int64_t *out_hist,
                         int64_t *out_rowsum, int32_t *out_edge, int32_t *out_counts, float *out_kernel_ms);

#define MI_COMPONENTS_GLOBAL 1u                     /* flags bit 0: the global form (parent array in HBM) at any n */
#define MI_COMPONENTS_LDS_MAX_CELLS 26624           /* n up to here runs with the parent array in LDS (see below) */
#define MI_COMPONENTS_MAX_ENTRIES (1ll << 32)       /* B * n (16 GiB of int32 output) */

/* Batched connected components of one undirected graph under a per-item edge filter.  rowptr (n + 1, rowptr[0] = 0,
 * monotone) and col (rowptr[n] entries in [0, n)): host CSR over n cells; B items.  The stored entry e = (i, col[e]) is live
 * in item b iff (L == NULL or L[b, i] == L[b, col[e]]) and (keep == NULL or keep[b, e] != 0); L is B x n uint16 (any
 * values), keep B x rowptr[n] bytes.  An edge connects its ends when it is live in at least one stored direction (storing
 * one direction only is enough); self loops connect nothing.  Outputs (host, caller-allocated):
 *   out_labels    B x n int32: the component of every cell, numbered 0 .. C_b - 1 in ascending order of each component's
 *                 smallest cell (the numbering of metrics.consensus_labels)
 *   out_count     B int32: C_b
 *   out_kernel_ms device time of the kernel, or NULL
 * A pure function of the input: it does not depend on the order in which the atomics land.
 * LDS plan of the primary form (one workgroup per item): the parent array, 4 B per cell, and the item's label row, 2 B
 * per cell, read once, beside 320 B of static LDS (the 16 wavefront totals of the final scan, 64 B, and the scratch of the
 * workgroup-wide "changed" vote); 6 n + 320 bytes <= 160 KB, rounded down to n <= MI_COMPONENTS_LDS_MAX_CELLS = 26 624 (one limit,
 * with or without labels).  Beyond it, or with MI_COMPONENTS_GLOBAL, the parent array is the item's own row of the output
 * in HBM (global atomics, one workgroup per item) and the labels are read from L2.
 * MI_EINVAL for NULL outputs, n < 1, B < 1, unknown flags, rowptr[0] != 0, a non-monotone rowptr, a col outside [0, n);
 * MI_EUNSUPPORTED for B * n > MI_COMPONENTS_MAX_ENTRIES; all before any device work. */
int mi_graph_components(const int32_t *rowptr, const int32_t *col, int n, const uint16_t *L, const uint8_t *keep, int B,
                        int device, uint32_t flags, int32_t *out_labels, int32_t *out_count, float *out_kernel_ms);

#define MI_MARKERS_SUM_PLAIN 1u                     /* flags bit 0: out_sum adds (double)x (scale.data, counts), not expm1 */
#define MI_MARKERS_GLOBAL    2u                     /* flags bit 1: every gene is ranked in the HBM form */
#define MI_MARKERS_LDS_MAX_NONZEROS 8192            /* a gene with at most this many non-zero cells is ranked in LDS */
#define MI_MARKERS_LABELLING_CHUNK 16               /* labellings scored per pass over a sorted gene */
#define MI_MARKERS_MAX_CELLS (1 << 20)              /* n: t^3 of a tie group of n cells must fit in int64 */
#define MI_MARKERS_MAX_ENTRIES (1ll << 28)          /* B * g * K (2 GiB of int64 output) */

/* Batched Wilcoxon rank-sum statistics.  X: n cells x g genes, row-major host array (the layout of cluster_stats), any
 * finite values (negatives allowed; -0.0 and +0.0 are both zero; values compare as floats).  L: B x n uint16 labellings,
 * labels in [0, K), K <= 64 (unused labels allowed).  The cells of a gene are ranked 1 .. n in ascending order of x, ties
 * sharing the mean of their ranks (midranks).  Outputs (host, caller-allocated; all but out_rank2 nullable):
 *   out_rank2     B x g x K int64: 2 * (sum of the midranks of the cells of cluster c), exact
 *   out_npos      B x g x K int32: cells of cluster c with x > 0
 *   out_sum       B x g x K double: sum over the cluster's cells, in ascending cell order, of expm1((double)x), or of
 *                 (double)x with MI_MARKERS_SUM_PLAIN; one thread per (labelling, gene) adds in that order, so the result
 *                 is a pure function of the input
 *   out_tie       g int64: sum over the gene's tie groups (the zeros included) of t^3 - t
 *   out_kernel_ms device time of the kernels
 * Three kernels: a tiled transpose of X into gene-major order; the ranking pass, one workgroup per gene (grid-stride):
 * the gene's non-zeros are compacted as (order-preserving key << 32 | cell) and sorted by a bitonic network, every sorted
 * position finds its tie run by binary search and stores its doubled midrank (first + last rank of the run; positives lie
 * behind the zero block, whose doubled midrank is 2 * negatives + zeros + 1), then MI_MARKERS_LABELLING_CHUNK labellings at a
 * time add it to their clusters with integer LDS atomics (the zero block's share of a cluster is its size minus its
 * non-zero cells); and the sums, one thread per (labelling, gene) walking the cells.
 * LDS plan of the ranking pass: 8 B per sorted entry and 4 B per doubled midrank, for the next power of two of the largest
 * non-zero count served in LDS, and 12 B per (labelling of the chunk, cluster): 12 * 8192 + 12 * 16 * 64 = 110 592 bytes of
 * the 160 KB at the cap, MI_MARKERS_LDS_MAX_NONZEROS = 8192 (16 384 entries would need 208 896).  A gene with more
 * non-zeros, or every gene with MI_MARKERS_GLOBAL, runs the same code on its workgroup's slab in HBM (the accumulators stay
 * in LDS).
 * MI_EINVAL for NULL X, L or out_rank2, n < 1, g < 1, B < 1, K outside [1, 64], unknown flags, a label >= K, a NaN or an
 * infinity in X; MI_EUNSUPPORTED for n > MI_MARKERS_MAX_CELLS and for B * g * K > MI_MARKERS_MAX_ENTRIES; all before any
 * device work. */
int mi_rank_sum_markers_f32(const float *X, int n, int g, const uint16_t *L, int B, int K, int device, uint32_t flags,
                            int64_t *out_rank2, int32_t *out_npos, double *out_sum, int64_t *out_tie,
                            float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_METRICS_H */
