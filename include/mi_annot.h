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
 * No floating-point atomics; two calls return identical bits.
 */
#ifndef MI_ANNOT_H
#define MI_ANNOT_H

#include <stdint.h>

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
 * is resident, and mi_annot_fine_tune returns MI_ESTATE until a later mi_annot_score succeeds. */
int mi_annot_score(mi_annot *h, const float *X, int n_c, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2,
                   double *out_scores, int32_t *out_first, float *out_kernel_ms);

/* The fine-tuning loop on the resident chunk.  Outputs, n_c entries each, nullable: out_labels, out_best / out_next (the
 * largest and second-largest of the last scores computed; -inf for out_next when L = 1), out_iterations.  MI_ESTATE when
 * no chunk is resident: before the first mi_annot_score, and after one that was refused or that failed. */
int mi_annot_fine_tune(mi_annot *h, int32_t *out_labels, double *out_best, double *out_next, int32_t *out_iterations,
                       float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_ANNOT_H */
