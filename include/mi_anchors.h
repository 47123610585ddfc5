/* mi_anchors.h -- anchor-based label and feature transfer on MI355X (gfx950): Seurat v4's FindTransferAnchors / TransferData as
 * this package specifies them ("chain A": DESIGN.md section 5d; numpy restatement: tests/anchor_reference.py).
 * Implemented in csrc/anchor_kernels.hip, exported by libmi_sa.so.  Return codes and mi_last_error(): mi_sa.h.
 *
 * Two point sets in one common space, the reference R (n x dim) and the query Q (m x dim):
 *   A0 (host)  with l2_norm every row is divided by its fp64 Euclidean norm (sum of squares in coordinate order) and rounded
 *              to f32; an all-zero row is MI_EINVAL.
 *   A1 (Q1)    K = max(k_anchor, k_score); four exact kNN tables by ascending (distance, index), nothing excluded: RR (n x K,
 *              reference in reference), RQ (n x K, reference in query), QR (m x K), QQ (m x K).  The search is chain Q's
 *              k_knn_cross (csrc/mapping_kernels.hip), called, not copied.
 *   A2         (r, q) is an anchor iff q is in RQ[r, :k_anchor] and r is in QR[q, :k_anchor]; anchors are listed by ascending r,
 *              then by q's rank in RQ[r] (k_anchor_pairs_count, an exclusive scan, k_anchor_pairs_fill: no atomics).
 *   A3         raw(r, q) = |S_r n S_q|, S_r = RR[r, :k_score] u (n + RQ[r, :k_score]), S_q = QR[q, :k_score] u (n + QQ[q, :k_score])
 *              (k_anchor_score: one wavefront per anchor, the four id lists in LDS).  The host turns raw into scores in [0, 1]
 *              and hands them back with mi_anchors_set_scores.
 *   A4 (Q1)    U = the distinct query cells of the anchors, ascending; for EVERY query cell its k_weight nearest rows of Q[U]
 *              (indices WN into U, f32 distances WD).
 *   A5         k_anchor_weights: one wavefront per query cell c; dk = WD[c, k_weight - 1]; for i = 0 .. k_weight - 1 and every
 *              anchor a of query cell U[WN[c, i]] in anchor-list order: t = (1 - WD[c, i] / dk) * score[a] (the ratio is 0 when
 *              dk = 0), w = -expm1(-t / (2 / sd_weight)^2), fp64; the row is divided by its sum taken in that order (a zero
 *              sum leaves a zero row).  A CSR over the query cells: rowptr, anchor, weight.
 *   A6         k_anchor_predict_labels / k_anchor_predict_features: fp64 sums over a row in row order.
 * Every sum has one order: two calls return the same bits.  A query's result depends on the other queries of the call (QQ and
 * RQ see them). */
#ifndef MI_ANCHORS_H
#define MI_ANCHORS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_anchors mi_anchors;

#define MI_ANCHORS_PASSES 5             /* pass_ms of mi_anchors_info: knn, pairs, score, weight_knn, weights */

/* A0 - A3 (the integer part).  R: n x dim, Q: m x dim, row-major finite f32, 1 <= dim <= 64;
 * 2 <= k_anchor <= K = max(k_anchor, k_score) <= min(n, m, 64), k_score >= 1; l2_norm 0 or 1.  The (normalised) points, the four
 * tables, the anchors, their raw scores and the anchors-by-query-cell lists stay resident in the handle.  MI_EINVAL for a
 * non-finite cell, an all-zero row under l2_norm or coordinate ranges mi_umap_query_knn_f32 refuses; MI_EUNSUPPORTED for n or
 * m > MI_UMAP_MAX_POINTS or (n + m) * K >= 2^30.  out_kernel_ms: the device time of all passes. */
int mi_anchors_find_f32(const float *R, int n, const float *Q, int m, int dim, int k_anchor, int k_score, int l2_norm,
                        int device, mi_anchors **out, float *out_kernel_ms);
int mi_anchors_destroy(mi_anchors *a);

/* n_anchors: A; n_anchor_queries: |U|; nnz: entries of the weight CSR (0 before mi_anchors_weights); device_bytes: what the
 * handle holds resident now (the scratch of a running pass is not the handle's); pass_ms: MI_ANCHORS_PASSES floats, the device
 * time of each pass as last run (0 for one that has not).  Each nullable. */
int mi_anchors_info(const mi_anchors *a, int *n_anchors, int *n_anchor_queries, int64_t *nnz, int64_t *device_bytes,
                    float *pass_ms);

/* pairs: A x 2 (reference cell, query cell); raw: A integers in [0, 2 k_score]; RR, RQ: n x K; QR, QQ: m x K.  Each nullable. */
int mi_anchors_fetch(mi_anchors *a, int32_t *pairs, int32_t *raw, int32_t *RR, int32_t *RQ, int32_t *QR, int32_t *QQ);

/* score: A finite values in [0, 1] (MI_EINVAL otherwise), one per anchor in list order.  Weights computed before are dropped. */
int mi_anchors_set_scores(mi_anchors *a, const double *score);

/* A4 - A5.  2 <= k_weight <= min(|U|, 64), sd_weight finite and > 0; MI_ESTATE before mi_anchors_set_scores;
 * MI_EUNSUPPORTED for m * k_weight * k_anchor >= 2^31 (the bound on the CSR's size). */
int mi_anchors_weights(mi_anchors *a, int k_weight, double sd_weight, float *out_kernel_ms);

/* rowptr: m + 1; anchor, weight: rowptr[m] entries (anchor: an index into the anchor list); wn: m x k_weight indices into U;
 * wd: m x k_weight f32 distances.  Each nullable.  MI_ESTATE before mi_anchors_weights. */
int mi_anchors_fetch_weights(mi_anchors *a, int64_t *rowptr, int32_t *anchor, double *weight, int32_t *wn, float *wd);

/* A6, labels.  labels: n codes, -1 = unlabelled, else in [0, L) (MI_EINVAL otherwise).  scores[c, l] = the sum of the row's weights
 * over the anchors whose reference cell has code l, fp64 in row order; label[c]: the largest score, ties to the smaller code,
 * -1 where no class has a positive score; score[c]: the winner's (0 with label -1).  scores: nullable dense m x L;
 * MI_EUNSUPPORTED for m * L >= 2^31.  MI_ESTATE before mi_anchors_weights. */
int mi_anchors_predict_labels(mi_anchors *a, const int32_t *labels, int L, int32_t *label, double *score, double *scores,
                              float *out_kernel_ms);

/* A6, features.  refdata: n x F finite f32; pred[c, f] = f32(sum_a w_a * (double)refdata[r_a, f]) over row c in row order, the
 * product and the sum rounded apart.  MI_EUNSUPPORTED for m * F >= 2^31.  MI_ESTATE before mi_anchors_weights. */
int mi_anchors_predict_features(mi_anchors *a, const float *refdata, int F, float *pred, float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_ANCHORS_H */
