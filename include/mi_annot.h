/*
 * mi_annot.h -- C ABI of reference-based cell-type annotation on MI355X (part of libmi_sa.so): Spearman scores of every
 * test cell against every reference sample on a set of marker genes, the per-label 0.8 quantile, and the per-cell
 * fine-tuning loop.  DESIGN.md section 5c ("chain A") is the specification.
 *
 * The LAST step of the reference's assessment notebook, in R (SingleR):
 *     R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:146-179, Pbmc3k_normalization_simulated_data.Rmd:377-412, 1071-1077
 *         SingleR(test = sce, ref = monaco.ref, labels = monaco.ref$label.main)
 * The chain here is modelled on SingleR's defaults (de.method = "classic", quantile = 0.8, fine.tune = TRUE, tune.thresh =
 * 0.05); agreement with R's SingleR is not pinned.  The markers (host fp64) and the pruning (host fp64) are in annotate.py.
 *
 * Conventions as in mi_prep.h: plain C types, an opaque handle, caller-allocated host outputs, 0 / negative MI_E* return
 * codes, mi_last_error() for the message, every argument check before any device work.  The handle holds the reference:
 * it is uploaded and ranked once, and the test cells arrive in chunks of at most MI_ANNOT_MAX_CHUNK.
 *
 * Kernels (csrc/annot_kernels.hip):
 *   k_annot_rank       one workgroup per row (a reference sample or a test cell): the doubled midranks r2 of the row over the
 *                      m marker genes (2 <= r2 <= 2 m; both zeros are one value), written as two base-128 digits in two i8
 *                      planes, and sum r2^2.
 *   k_annot_cross      sum a b for all (cell, sample) pairs on v_mfma_i32_16x16x64_i8: the four digit products in i32,
 *                      combined as 16384 hh + 128 (hl + lh) + ll in int64.  Exact.
 *   k_annot_scores     one workgroup per cell: rho per sample in fp64 from the integers, the 0.8 quantile per label, the argmax.
 *   k_annot_fine_tune  one workgroup per cell: the loop of DESIGN.md section 5c on the genes G' of the labels still in use.
 *
 * The test cells may also come from a resident mi_prep_matrix (include/mi_prep.h), dense or sparse, with no n x g host
 * traffic: mi_annot_score_matrix gathers a row range of the handle on the marker genes into the chunk, and
 * mi_annot_score_clusters (SingleR's clusters = mode) fills the chunk with one averaged profile per cluster.
 *   k_annot_gather_dense  chunk[i][s] = V[(row0 + i) g + cols[s]], 64-bit element indices.
 *   k_annot_gather_csr    one workgroup per cell: m zeros in LDS, the cell's stored entries whose gene has a slot written
 *                         over their slot, one coalesced store of the row.
 *   k_annot_means<Src>    one wavefront per (marker gene, block of 64 clusters), lane = cluster: the gene's entries in
 *                         ascending cell order (a dense column, or the stored entries of the transpose), each added in fp64 by
 *                         the lane whose cluster owns the cell; mean = (float)(sum / size).
 * Everything after the gather is the chain above on the chunk.
 * No floating-point atomics; two calls return identical bits.
 */
#ifndef MI_ANNOT_H
#define MI_ANNOT_H

#include <stdint.h>

#include "mi_prep.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_annot mi_annot;

#define MI_ANNOT_MAX_GENES    8191          /* m: 2 m < 128^2, two base-128 digits hold a doubled midrank */
#define MI_ANNOT_MAX_LABELS   64            /* L */
#define MI_ANNOT_MAX_SAMPLES  4096          /* S */
#define MI_ANNOT_MAX_CHUNK    16384         /* n_c of one mi_annot_score call */

/* R: S x m row-major f32, the reference restricted to the marker genes; labels: S label ids in [0, L), every id used;
 * pair_masks: L * L rows of ceil(m / 32) words, bit j of row a * L + b set when gene j is a marker of the ordered pair
 * (a, b) (the diagonal rows are ignored).  Uploads them and ranks the samples.  out_kernel_ms (nullable): the ranking
 * kernel.  MI_EINVAL for NULL arguments, a label outside [0, L), a label without samples, a NaN or infinity in R, a mask
 * bit at or past m; MI_EUNSUPPORTED for m outside [1, MI_ANNOT_MAX_GENES], L outside [1, MI_ANNOT_MAX_LABELS], S outside
 * [L, MI_ANNOT_MAX_SAMPLES]. */
int mi_annot_create(const float *R, int S, int m, const int32_t *labels, int L, const uint32_t *pair_masks, int device,
                    mi_annot **out, float *out_kernel_ms);
int mi_annot_destroy(mi_annot *h);

/* X: n_c x m row-major f32, a chunk of test cells on the marker genes; it stays resident for mi_annot_fine_tune.  Outputs,
 * each nullable: out_sab n_c x S (sum a b, samples in the caller's order), out_sa2 n_c, out_sb2 S, out_scores n_c x L fp64,
 * out_first n_c (argmax of the scores, lowest label on ties); out_kernel_ms: 3 floats, the ranking, cross and score
 * kernels.  MI_EINVAL for NULL h or X, n_c < 1, a NaN or infinity in X; MI_EUNSUPPORTED for n_c > MI_ANNOT_MAX_CHUNK.
 * Every call with a handle first drops the chunk of the call before: after a call that was refused or that failed, no chunk
 * is resident, and mi_annot_fine_tune returns MI_ESTATE until a later mi_annot_score* call succeeds. */
int mi_annot_score(mi_annot *h, const float *X, int n_c, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2,
                   double *out_scores, int32_t *out_first, float *out_kernel_ms);

/* The fine-tuning loop on the resident chunk.  Outputs, n_c entries each, nullable: out_labels, out_best / out_next (the
 * largest and second-largest of the last scores computed; -inf for out_next when L = 1), out_iterations.  MI_ESTATE when
 * no chunk is resident: before the first mi_annot_score* call, and after one that was refused or that failed. */
int mi_annot_fine_tune(mi_annot *h, int32_t *out_labels, double *out_best, double *out_next, int32_t *out_iterations,
                       float *out_kernel_ms);

/* mi_annot_score on rows [row0, row0 + n_c) of a resident expression handle, restricted to the genes `cols` (m indices in
 * [0, g), any order, no repeats: the handle's positions of the annotator's m marker genes); which: 0 the uploaded values,
 * 1 the output of mi_prep_normalize (MI_PREP_MARKERS_COUNTS / _NORMALIZED).  The chunk is gathered on the device and stays
 * resident for mi_annot_fine_tune; the outputs are those of mi_annot_score on the densified slice, bit for bit (a stored
 * zero of a sparse handle is a zero).  out_kernel_ms: 4 floats, the gather, ranking, cross and score kernels.
 * The checks, all before any device work and in this order: NULL h (MI_EINVAL; from here on no chunk is resident until a
 * call succeeds); NULL M or cols; which outside {0, 1}; M on another device than h; row0 < 0, n_c < 1 or row0 + n_c > n
 * (all MI_EINVAL); n_c > MI_ANNOT_MAX_CHUNK (MI_EUNSUPPORTED); a column outside [0, g) or repeated (MI_EINVAL); which = 1
 * before mi_prep_normalize (MI_ESTATE).  M is not modified and all scratch outside the annotator is freed on return:
 * mi_prep_info's device_bytes is the same before and after. */
int mi_annot_score_matrix(mi_annot *h, mi_prep_matrix *M, int which, const int32_t *cols, int row0, int n_c, int64_t *out_sab,
                          int64_t *out_sa2, int64_t *out_sb2, double *out_scores, int32_t *out_first, float *out_kernel_ms);

/* SingleR's clusters = mode: the chunk becomes K rows, row c the mean profile of the cells i with cluster_of[i] == c (n
 * entries in [0, K), every cluster used) on the genes `cols`, and the chain runs on it with n_c = K.  The specification of
 * a mean: sum = the fp64 sum of (double)x[i][cols[s]] over the cluster's cells in ascending cell index, one addition after
 * another; mean = (float)(sum / (double)size).  A sparse handle walks only the stored entries of the gene (zeros add +0.0
 * to a non-negative sum) and returns the dense handle's bits.  out_sizes (K, nullable): the cells per cluster; the five
 * outputs as mi_annot_score with n_c = K; out_kernel_ms: 4 floats, the means, ranking, cross and score kernels.
 * The checks, in this order: those of mi_annot_score_matrix up to the device; NULL cluster_of, K < 1 (MI_EINVAL); K >
 * MI_ANNOT_MAX_CHUNK (MI_EUNSUPPORTED); the columns; a cluster_of entry outside [0, K), a cluster without cells
 * (MI_EINVAL); the state.  M is not modified, as above. */
int mi_annot_score_clusters(mi_annot *h, mi_prep_matrix *M, int which, const int32_t *cols, const int32_t *cluster_of, int K,
                            int32_t *out_sizes, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2, double *out_scores,
                            int32_t *out_first, float *out_kernel_ms);

/* The resident chunk as the chain reads it: n_c x m f32 (the gathered cells, the K mean rows, or the X of mi_annot_score).
 * MI_EINVAL for a NULL argument, MI_ESTATE when no chunk is resident. */
int mi_annot_fetch_chunk(mi_annot *h, float *out);

#ifdef __cplusplus
}
#endif
#endif /* MI_ANNOT_H */
