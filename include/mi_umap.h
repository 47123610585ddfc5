/*
 * mi_umap.h -- C ABI of UMAP on MI355X (part of libmi_sa.so): exact kNN with distances -> smooth kNN distances -> fuzzy
 * union graph -> a deterministic SGD layout.  DESIGN.md section 5d ("chain U") is the specification.
 *
 * The step AFTER the clustering in every notebook of the reference, in R (Seurat):
 *     R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:94-108, R/kidney/Kidney_data.Rmd:133-155,183, Kidney_subsampling.Rmd:47,86
 *         RunUMAP(obj, dims = 1:15) -> DimPlot(reduction = "umap", group.by = ...)
 * Seurat hands that to uwot / umap-learn, whose layout is a racy Hogwild loop: two runs differ.  Here every epoch is a
 * GATHER -- each vertex sums its own forces from the previous epoch's positions, negatives come from a counter-based
 * Philox, nothing is accumulated with floating-point atomics -- so two runs are bit-identical.
 *
 * Conventions as in mi_prep.h: plain C types, an opaque handle, caller-allocated host outputs, 0 / negative MI_E* return
 * codes, mi_last_error() for the message, every argument check before any device work, and a nullable
 * `float *out_kernel_ms` (HIP event time of the pass's kernels only) on each pass.
 *
 * Kernels (csrc/umap_kernels.hip):
 *   U1 k_knn (csrc/snn_kernels.hip, unchanged) then k_umap_dist: one thread per (point, neighbour) recomputes the squared
 *      distance with k_knn's f32 fmaf chain (coordinates in ascending order) and turns it into the metric's distance.
 *   U2 k_umap_rho: one thread per point, rho_i and the fp64 mean of its k distances; the host adds the n means in index
 *      order (mean_all); k_umap_sigma: one thread per point, exactly 64 bisection steps in fp64.
 *   U3 reverse-neighbour lists (k_rn_count / k_scan_exclusive / k_rn_fill of snn_kernels.hip), then k_umap_union_raw: one
 *      wavefront per row, one lane per candidate (the row's k - 1 neighbours, then the points that list it), fp64 weights,
 *      a row of any length loops; k_umap_union_sort: each surviving entry's place is the number of smaller columns in its
 *      row (rank by counting: the rows come out ascending whatever order the reverse lists were filled in).  w_max by an
 *      integer atomicMax on the bits of the positive floats.
 *   U4 k_umap_layout<G, C>: one launch per epoch on one stream, no host synchronisation between epochs.  A group of G
 *      lanes (16, 32 or 64: the smallest that holds the mean row length, a function of the graph alone) owns a vertex;
 *      lane l takes entries l, l + G, ... of the row in ascending order, each with its negatives; the G partial sums meet in
 *      a butterfly of xor-shuffles.  Y_t is read, Y_{t+1} written: two buffers.
 */
#ifndef MI_UMAP_H
#define MI_UMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_umap_graph mi_umap_graph;

#define MI_UMAP_EUCLIDEAN   0
#define MI_UMAP_COSINE      1
#define MI_UMAP_MAX_POINTS  (1 << 23)       /* n */
#define MI_UMAP_MAX_EPOCHS  10000           /* T of mi_umap_layout_f32 */
#define MI_UMAP_MAX_NEGATIVE 16             /* neg of mi_umap_layout_f32 */

/* U1.  X: n x dim row-major f32 (finite), 1 <= dim <= 64; k = n_neighbors, the point itself counts: 2 <= k <= 64, k <= n.
 * metric MI_UMAP_EUCLIDEAN: d = sqrtf(d2).  MI_UMAP_COSINE: every row is first divided by its norm on the host (fp64 sum of
 * squares in coordinate order, sqrt, fp64 quotient rounded to f32; an all-zero row stays zero), the search is euclidean
 * on those rows and d = d2 / 2 (= 1 - cos up to rounding, and the same ordering).  MI_EINVAL for NULL arguments, the ranges
 * above, an unknown metric, a non-finite coordinate, or coordinate ranges r_c = max_i x_ic - min_i x_ic with sum_c r_c^2 >
 * FLT_MAX / 2 (an fp32 squared distance could overflow and the point would get no neighbour; the same rule as mi_snn.h,
 * applied to the rows the search sees, so the cosine metric always passes it); MI_EUNSUPPORTED for n > MI_UMAP_MAX_POINTS or
 * n * k >= 2^30. */
int mi_umap_knn_f32(const float *X, int n, int dim, int k, int metric, int device, mi_umap_graph **out,
                    float *out_kernel_ms);
int mi_umap_destroy(mi_umap_graph *g);
/* nn: n x k indices exactly as mi_snn_fetch returns them (column 0 = the point, then ascending (d2, index)); dist: n x k
 * f32, column 0 is 0.  Each nullable. */
int mi_umap_fetch_knn(mi_umap_graph *g, int32_t *nn, float *dist);

/* U2.  rho_i = the smallest positive distance of the row (0 if none); sigma_i by 64 bisection steps to
 * sum_{j >= 1} exp(-max(d_ij - rho_i, 0) / sigma) = log2(k), floored at 1e-3 * (the row's mean distance if rho_i > 0, else the
 * mean of all rows' means). */
int mi_umap_smooth(mi_umap_graph *g, float *out_kernel_ms);
/* rho, sigma: n fp64 entries each (nullable).  MI_ESTATE before mi_umap_smooth. */
int mi_umap_fetch_smooth(mi_umap_graph *g, double *rho, double *sigma);

/* U3.  w_ij = v_ij + v_ji - v_ij v_ji in fp64, stored as f32; entries whose stored weight is 0 are dropped.  The result is a
 * symmetric CSR: rows ascending by column, no diagonal, w_ij == w_ji bit for bit.  MI_ESTATE before mi_umap_smooth. */
int mi_umap_union(mi_umap_graph *g, float *out_kernel_ms);
/* each pointer nullable; nnz, max_degree and w_max are 0 before mi_umap_union */
int mi_umap_info(const mi_umap_graph *g, int *n, int *k, int64_t *nnz, int *max_degree, float *w_max);
/* rowptr n + 1, col / w nnz entries (each nullable).  MI_ESTATE before mi_umap_union. */
int mi_umap_fetch_graph(mi_umap_graph *g, int64_t *rowptr, int32_t *col, float *w);

/* U4, on ANY symmetric CSR (rowptr n + 1, col / w rowptr[n] entries): the handle's graph, or e.g. a trimmed SNN graph with its
 * Jaccard weights.  Y0, Y_out: n x c row-major f32; a, b: the curve constants; alpha0: the initial learning rate; T epochs;
 * neg negative samples per firing edge; seed: the Philox key.  The rows are used as given: symmetry is the caller's
 * business.  MI_EINVAL for NULL arguments, n < 1, rowptr[0] != 0 or a decreasing rowptr, columns of a row not strictly
 * ascending or outside [0, n), a diagonal entry, a non-finite or non-positive weight, T < 1 or T > MI_UMAP_MAX_EPOCHS,
 * neg < 0 or neg > MI_UMAP_MAX_NEGATIVE, a non-finite Y0 / a / b / alpha0; MI_EUNSUPPORTED for c not 2 or 3, n >
 * MI_UMAP_MAX_POINTS or rowptr[n] >= 2^32. */
int mi_umap_layout_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *w, const float *Y0, float a,
                       float b, float alpha0, int T, int neg, uint64_t seed, int device, float *Y_out,
                       float *out_kernel_ms);

/* ---- chain Q: mapping new points onto a fixed reference (csrc/mapping_kernels.hip) --------------------
 * Exact kNN of a query set against ANOTHER set, then umap-learn's transform rule on those rows: a weighted neighbour vote
 * (label transfer), the weighted-mean start and the out-of-sample layout.  A query's results depend on the reference and on
 * that query alone: never on which other queries are sent with it.
 *
 * Kernels:
 *   Q1 k_knn_cross<DP, KM>: k_knn with the queries and the streamed set apart (one query per thread, the reference through an
 *      LDS tile every lane reads at the same address, top-KM list in registers, KM in {8, 16, 32, 64} >= k; nothing excluded),
 *      then k_query_dist.  One wavefront per 64 queries: a small m against a large n leaves most CUs idle.
 *   Q2 k_query_smooth: one thread per query, sigma (64 bisection steps, rho = 0, all k columns) and the k weights.
 *   Q3 k_query_init<C>, Q5 k_query_vote: one thread per query, fp64 sums in column order.
 *   Q4 k_umap_transform<G, C>: ALL T epochs in one launch.  A group of G lanes (16, 32 or 64: the smallest >= k) owns a query;
 *      lane l holds entry l; neighbour, firing ratio and the query's position stay in registers across the epochs. */
typedef struct mi_umap_query mi_umap_query;

/* Q1.  R: n x dim (the reference), Q: m x dim (the queries), row-major finite f32; 1 <= dim <= 64, n >= 2, m >= 1,
 * 2 <= k <= min(64, n).  The k neighbours of a query are ordered by ascending (d2, index); nothing is excluded (a query equal to
 * a reference point finds it at distance 0).  Metrics, the cosine row normalisation (of both sets) and the distances are
 * mi_umap_knn_f32's; its coordinate-range rule is applied with the ranges taken over R and Q together.  MI_EUNSUPPORTED for n or
 * m > MI_UMAP_MAX_POINTS or m * k >= 2^30. */
int mi_umap_query_knn_f32(const float *R, int n, const float *Q, int m, int dim, int k, int metric, int device,
                          mi_umap_query **out, float *out_kernel_ms);
int mi_umap_query_destroy(mi_umap_query *q);
/* nn: m x k indices into R; dist: m x k f32, ascending in each row.  Each nullable. */
int mi_umap_query_fetch_knn(mi_umap_query *q, int32_t *nn, float *dist);

/* Q2.  sigma_i by U2's 64 bisection steps to sum_{p < k} (d_ip > 0 ? exp(-d_ip / sigma) : 1) = log2(k) (rho = 0, every column),
 * floored at 1e-3 * the row's OWN mean distance; v_ip = (d_ip > 0 ? exp(-d_ip / sigma_i) : 1) in fp64, stored as f32. */
int mi_umap_query_smooth(mi_umap_query *q, float *out_kernel_ms);
/* sigma: m fp64 entries, w: m x k f32 (each nullable).  MI_ESTATE before mi_umap_query_smooth. */
int mi_umap_query_fetch_smooth(mi_umap_query *q, double *sigma, float *w);

/* Q5.  labels: n entries, -1 = unlabelled, else in [0, L) (MI_EINVAL otherwise).  weighted 0: every labelled neighbour counts
 * 1; weighted 1: it counts v_ip (MI_ESTATE before mi_umap_query_smooth).  score(l) = the share of label l in the labelled
 * neighbours' total, fp64 in column order; label: the largest score, ties to the smaller label; score: the winner's.  A row
 * whose labelled neighbours weigh nothing in all (none is labelled, or every weight is 0) gets label -1 and score 0.
 * scores: nullable dense m x L fp64 (zeros included); MI_EUNSUPPORTED for m * L >= 2^31. */
int mi_umap_query_vote(mi_umap_query *q, const int32_t *labels, int L, int weighted, int32_t *label, double *score,
                       double *scores, float *out_kernel_ms);

/* Q3.  Yref: n x c f32 (finite), c 2 or 3 (else MI_EUNSUPPORTED); Y0_i = sum_p v_ip Yref[nn_ip] / sum_p v_ip, fp64 in column
 * order on the stored weights, rounded to f32.  MI_ESTATE before mi_umap_query_smooth. */
int mi_umap_query_init(mi_umap_query *q, int c, const float *Yref, float *Y0, float *out_kernel_ms);

/* Q4 on plain arrays: m queries of k entries each (nn: m x k indices into Yref's n rows, w: m x k weights), 1 <= k <= 64.  Only
 * the queries move.  Entry (i, p) fires by U4's test on the ratio w_ip / max_p w_ip (one f32 division by the ROW's largest
 * weight); a firing entry adds U4's attractive term toward Yref[nn_ip] and `neg` repulsive terms from Yref[j],
 * j = philox4x32_10(q0 + i, p, t, q; seed)[0] % n, with no index skipped.  alpha_t is U4's.  q0: the index of the first query
 * (rows a .. b of a larger call are reproduced bit for bit by a call on those rows with q0 = a).  MI_EINVAL for NULL
 * arguments, m or n < 1, k outside [1, 64], an nn outside [0, n), a weight that is not finite and >= 0, a row without a positive
 * weight, T / neg outside mi_umap_layout_f32's limits, non-finite Yref / Y0 / a / b / alpha0, q0 < 0 or q0 + m > 2^31 - 1;
 * MI_EUNSUPPORTED for c not 2 or 3, n or m > MI_UMAP_MAX_POINTS or m * k >= 2^30. */
int mi_umap_transform_layout_f32(int m, int k, const int32_t *nn, const float *w, int n, int c, const float *Yref,
                                 const float *Y0, float a, float b, float alpha0, int T, int neg, uint64_t seed, int64_t q0,
                                 int device, float *Y_out, float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_UMAP_H */
