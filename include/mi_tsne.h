/*
 * mi_tsne.h -- C ABI of t-SNE on MI355X (part of libmi_sa.so): exact kNN in passes of 64 -> perplexity calibration -> the joint
 * distribution P as a symmetric CSR -> a layout whose repulsion is exact.  DESIGN.md section 5d ("chain T") is the
 * specification, tests/tsne_reference.py restates it in numpy.
 *
 * The twin of the UMAP picture in the reference's normalisation notebook, in R (Seurat):
 *     R/pbmc3k/Pbmc3k_normalization_simulated_data.Rmd:236-237, 254-255, 272-273, 498
 *         RunUMAP(obj, reduction = "pca", dims = 1:10);  RunTSNE(obj, reduction = "pca", dims = 1:10)
 * Seurat hands that to Rtsne (bhtsne): Barnes-Hut repulsion at theta = 0.5.  Here every iteration is a GATHER -- each point sums
 * its own n - 1 Student-t terms from the previous iteration's positions in a fixed order, nothing is accumulated with
 * floating-point atomics -- so two runs are bit-identical, and the repulsion is exact (theta = 0).
 *
 * Conventions as in mi_umap.h: plain C types, an opaque handle that owns its device buffers, caller-allocated host outputs,
 * 0 / negative MI_E* return codes, mi_last_error() for the message, every argument check before any device work, and a
 * nullable `float *out_kernel_ms` (HIP event time of the pass's kernels only) on each pass.
 *
 * Kernels (csrc/tsne_kernels.hip):
 *   T1 k_knn_after<DP>: k_knn_cross's structure (one query per thread, candidates through an LDS tile, top-64 in registers) with
 *      a per-query floor (d2, index): pass p collects neighbours 64 p .. 64 p + 63 (0-based), everything not lexicographically
 *      above the last entry of pass p - 1 is skipped, and so is the point itself.  ceil(K / 64) passes.
 *   T2 k_tsne_calibrate: one thread per point, exactly 100 steps of van der Maaten's bisection in fp64.
 *   T3 reverse-neighbour lists (snn_kernels.hip), k_tsne_joint_raw (one wavefront per row, one lane per candidate),
 *      k_tsne_joint_sort (rank by counting).
 *   T4 k_tsne_repulse<C> (all pairs; the j axis in S(n) chunks) and k_tsne_update<G, C> (a lane group per point: attraction,
 *      gain / momentum rule, Y_{t+1}): two launches per iteration on one stream, no host synchronisation between iterations.
 */
#ifndef MI_TSNE_H
#define MI_TSNE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_tsne_graph mi_tsne_graph;

#define MI_TSNE_MAX_POINTS  (1 << 18)       /* n: the repulsion is n^2 per iteration */
#define MI_TSNE_MAX_ITERS   10000           /* T of mi_tsne_layout_f32 */
#define MI_TSNE_MIN_PERPLEXITY 2.0
#define MI_TSNE_MAX_PERPLEXITY 85.0         /* K = floor(3 * perplexity) <= 255 */
#define MI_TSNE_CALIBRATION_STEPS 100

/* T1.  X: n x dim row-major f32 (finite), 1 <= dim <= 64.  K = floor(3 * perplexity) nearest OTHER points of every point by
 * squared euclidean distance in f32 (k_knn's fmaf chain over the coordinates in ascending order), ordered by ascending
 * (d2, index); exact.  MI_EINVAL for NULL arguments, n < 2, dim outside [1, 64], a perplexity outside [2, 85] (or NaN), K > n - 1
 * (Rtsne's "perplexity is too large"), a non-finite coordinate, or the coordinate-range rule of mi_snn.h (sum_c r_c^2 >
 * FLT_MAX / 2); MI_EUNSUPPORTED for n > MI_TSNE_MAX_POINTS.  X is used as given: Rtsne's centring and scaling of the input is
 * not applied (the calibrated P does not depend on either). */
int mi_tsne_knn_f32(const float *X, int n, int dim, double perplexity, int device, mi_tsne_graph **out,
                    float *out_kernel_ms);
int mi_tsne_destroy(mi_tsne_graph *g);
/* nn: n x K indices, d2: n x K f32 squared distances, ascending (d2, index) in each row.  Each nullable. */
int mi_tsne_fetch_knn(mi_tsne_graph *g, int32_t *nn, float *d2);

/* T2.  Per point, in fp64 on D_j = d2_ij - d2_i1 (the row shifted by its minimum): p_j = exp(-beta D_j), Z = sum p_j,
 * H = log Z + beta sum p_j D_j / Z, sums in column order.  beta starts at 1 with bounds -inf, +inf; a step: H > log(perplexity)
 * raises beta (lower bound = beta; doubled while the upper bound is infinite, else the midpoint), otherwise lowers it
 * symmetrically.  Exactly MI_TSNE_CALIBRATION_STEPS steps, no tolerance exit; the conditional row p_j|i = p_j / Z is evaluated
 * at the beta the last step left.  A row whose D is all zero has H = log K > log(perplexity) at every beta: it stays uniform
 * and beta ends at 2^100. */
int mi_tsne_calibrate(mi_tsne_graph *g, float *out_kernel_ms);
/* beta: n fp64, cond: n x K conditional probabilities rounded to f32 (each nullable).  MI_ESTATE before mi_tsne_calibrate. */
int mi_tsne_fetch_calibration(mi_tsne_graph *g, double *beta, float *cond);

/* T3.  P_ij = (p_j|i + p_i|j) / (2 n) over the union of the kNN pattern, in fp64, stored as f32; entries whose stored value is
 * 0 are dropped.  A symmetric CSR: rows ascending by column, no diagonal, P_ij == P_ji bit for bit.  MI_ESTATE before
 * mi_tsne_calibrate. */
int mi_tsne_symmetrize(mi_tsne_graph *g, float *out_kernel_ms);
/* each pointer nullable; nnz and max_degree are 0 before mi_tsne_symmetrize */
int mi_tsne_info(const mi_tsne_graph *g, int *n, int *K, int64_t *nnz, int *max_degree);
/* rowptr n + 1, col / P nnz entries (each nullable).  MI_ESTATE before mi_tsne_symmetrize. */
int mi_tsne_fetch_graph(mi_tsne_graph *g, int64_t *rowptr, int32_t *col, float *P);

/* T4, on ANY symmetric CSR with positive finite weights (rowptr n + 1, col / P rowptr[n] entries).  Y: n x c row-major f32, c 2
 * or 3; U (velocity) and gains: n x c f32 or NULL (= 0 and 1).  Iteration t = t0 .. t0 + T - 1, all in f32 but Z:
 *     q_ij = 1 / (1 + |y_i - y_j|^2)                      Z = sum_{i != j} q_ij   (fp64 over f32 chunk sums)
 *     g_i  = e_t sum_{j in row i} P_ij q_ij (y_i - y_j) - (sum_{j != i} q_ij^2 (y_i - y_j)) / Z          (bhtsne: no factor 4)
 *     e_t  = exaggeration if t < exaggeration_iters else 1
 *     gain = gain + 0.2 if sign(g) != sign(u) else gain * 0.8, floored at 0.01                          (sign(0) = 0)
 *     u    = m_t u - (eta gain) g,  m_t = momentum0 if t < momentum_switch_iter else momentum1;        y = y + u
 * center != 0: after the LAST iteration of the call the fp64 column means of Y (index order), rounded to f32, are subtracted
 * from Y_out (not every iteration as Rtsne does: only differences enter the forces); U is untouched.  Resuming: a call of T
 * iterations equals a call of T1 with center = 0 followed by a call of T - T1 with t0 + T1 and the first call's Y_out, U_out,
 * gains_out, bit for bit.  Y_out n x c; U_out, gains_out (n x c) and Z_out (fp64: the last iteration's Z) nullable.
 * MI_EINVAL for NULL arguments, n < 2, what mi_umap_layout_f32 refuses in a CSR (rowptr[0] != 0, a decreasing rowptr, columns not
 * strictly ascending or outside [0, n), a diagonal entry, a weight that is not finite and positive), T outside [1,
 * MI_TSNE_MAX_ITERS], t0 < 0, non-finite Y / U / gains / eta / exaggeration / momentum or a gain <= 0; MI_EUNSUPPORTED for c not 2
 * or 3, n > MI_TSNE_MAX_POINTS or rowptr[n] >= 2^31.  Two refusals come AFTER the device work, when Y_out may already hold
 * what the run left: MI_EINVAL if the last iteration's Z is not finite and positive (every pair so far apart that |y_i - y_j|^2
 * overflowed f32 and q rounded to 0: the step divided by it) or if a coordinate of the result is not finite. */
int mi_tsne_layout_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *P, const float *Y,
                       const float *U, const float *gains, float eta, float exaggeration, int exaggeration_iters,
                       float momentum0, float momentum1, int momentum_switch_iter, int T, int t0, int center, int device,
                       float *Y_out, float *U_out, float *gains_out, double *Z_out, float *out_kernel_ms);

/* KL(P || Q) = sum_{stored} P_ij log(P_ij Z / q_ij) at Y: q and Z as in T4, every row's sum in fp64 in column order, the rows
 * added in index order: bit-identical between runs (Rtsne's final `itercosts`, summed).  Arguments checked as T4's. */
int mi_tsne_kl_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *P, const float *Y, int device,
                   double *kl, float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_TSNE_H */
