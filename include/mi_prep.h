/*
 * mi_prep.h -- C ABI of the preprocessing front end on MI355X (part of libmi_sa.so): counts -> log-normalised matrix ->
 * variable-gene statistics -> scaled matrix -> Gram matrix and PCA projection.
 *
 * The step BEFORE mi_snn.h.  In the reference it is the first chunk of every data-preparation notebook, in R (Seurat):
 *     R/pbmc3k/Pbmc3k_normalization_simulated_data.Rmd:81-82,184-185,488-492
 *         NormalizeData(LogNormalize, 1e4) -> FindVariableFeatures("vst", nfeatures) -> ScaleData -> RunPCA
 *     R/pbmc3k/Pbmc3k_prepare_data_for_QA_clustering.Rmd:51-52, R/kidney/Kidney_data.Rmd:47-48   the same RunPCA
 * followed directly by FindNeighbors(dims = 1:dim), which is mi_snn_build_f32.  The passes over the n x g matrix and the
 * O(n h^2) products run here; the loess curve of `vst` and the h x h eigen-solve stay on the host in fp64
 * (scrna_seq_qannealing_clustering_amd/preprocess.py).  DESIGN.md section 5c.
 *
 * Conventions as in mi_sa.h / mi_snn.h: plain C types, an opaque handle uploaded once, caller-allocated host outputs,
 * 0 / negative MI_E* return codes, mi_last_error() for the message, every argument check before any device work, and a
 * nullable `float *out_kernel_ms` (HIP event time of the pass's kernels only) on each pass.
 *
 * Layouts and kernels (csrc/prep_kernels.hip):
 *   X, Y     n cells x g genes, row-major f32 (the layout of mi_jaccard_cluster_stats and mi_rank_sum_markers_f32);
 *            element index 64-bit everywhere.
 *   k_prep_normalize    one wavefront per cell: the cell's total in fp64 (lane-strided, then a butterfly: a fixed order),
 *                       then y = (float) log1p((double) x * scale_factor / total).  No LDS.
 *   k_prep_col_partial<Mode>  column reductions: a workgroup is 64 genes x 4 row lanes over a slice of MI_PREP_ROW_SLICE
 *                       rows (reads coalesce along the genes); the 4 lanes meet in 2 KB (+ 1 KB for the counts) of LDS in
 *                       lane order; one fp64 partial per (slice, gene).  k_prep_col_finish adds the slices in ascending
 *                       order.  The slicing depends on n alone, so every result is a pure function of the input.  The mode
 *                       is the term, written once for both kinds of handle: ColSum, ColLog1p, ColCentred, ColClipped,
 *                       RegressMoment<0 / 1> and SctMoment<0 / 1> (the last two pairs: a residual, or its square about a mean).
 *   k_prep_select       one thread per element of Z: gathers the chosen columns of Y and scales them.  Z is n x ldz f32 with
 *                       ldz = h rounded up to 128, the padding columns zero.
 *   k_prep_gram         G = Z^T Z on v_mfma_f32_32x32x2_f32.  Work unit = (128 x 128 tile of the upper block triangle, chunk
 *                       of MI_PREP_GRAM_CHUNK cells); workgroup = 2 x 2 wavefronts, 64 x 64 each as 2 x 2 accumulators.  The
 *                       cells are the k index: 32 cells x 128 features of each of the two column blocks are staged in LDS as
 *                       [cell][128] floats (2 x 16 KB; lane l reads [k + (l >> 5)][tile + (l & 31)], conflict-free, and
 *                       Z's rows are already in that order, so no transpose is needed); a diagonal tile stages one block
 *                       and skips its lower-left wavefront.  The next 32 cells are fetched into registers while the MFMAs
 *                       of the current ones run.  A unit's f32 tile goes to a workspace;
 *   k_prep_gram_reduce  adds the chunks' tiles in fp64 in ascending chunk order and writes each entry and its mirror.
 *                       No floating-point atomics anywhere: two runs are bit-identical, G is exactly symmetric.
 *   k_prep_project      out = Z V on the same MFMA.  Workgroup = 64 cells x 128 output columns, wavefront w owns columns
 *                       32 w .. 32 w + 31 with two accumulators (cells 0-31, 32-63); 32 features per step: Z's tile, the
 *                       transposed operand (lane l needs Z[cell l & 31][k + (l >> 5)]), sits in LDS as [cell][33] floats
 *                       (odd stride: the 32 cells of a half-wave fall in 32 different banks), V's as [k][128]; 8.25 + 16 KB.
 *                       f32 accumulation over all h in feature order.
 *
 * Sparse input (mi_prep_create_csr_f32): the second kind of handle keeps the counts as CSR (int64 row pointers, int32
 * columns, f32 values) and the transpose as a position map (per gene: its rows, ascending, and the CSR position of each
 * entry), so one value array in the caller's order serves the per-cell and the per-gene walks; the normalised values are a
 * second value array of the same structure.  Resident memory is O(nnz + n + g + n ldz): no n x g buffer exists and n * g
 * is not limited.  CONTRACT: every output of a sparse handle equals, bit for bit, that of a dense handle on the densified
 * matrix -- the kernels add in the dense kernels' order (csrc/prep_kernels.hip, DESIGN.md section 5c "Sparse input"):
 *   k_prep_csr_normalize    one wavefront per cell, 64 entries at a time, each broadcast (v_readlane) to the lane
 *                           `column & 63`, columns ascending; the same butterfly; y for the stored entries only.  No LDS.
 *   k_prep_csc_col_partial<Term>  the workgroup and slice of k_prep_col_partial on the transpose: a thread finds its gene's
 *                           first entry of the slice by a lower bound in the gene's row list, and a zero's term is the dense
 *                           mode's own term function of 0.0f.  SumTerm and Log1pTerm add the stored entries; CentredTerm and
 *                           ClippedTerm walk every row of the slice and add the stored value's term or the per-gene constant
 *                           of a zero ((0 - mean)^2, min((0 - mean) / sd, clip)^2) at that row's place: sparse in memory,
 *                           n * g fp64 additions in arithmetic (the closed form (n - nnz) c gives other bits).
 *   k_prep_csr_select<Cols> one workgroup per cell builds its row of Z in LDS (ldz <= 4096 floats, 16 KB): every column's
 *                           value of y = 0, a barrier, the cell's stored entries of chosen genes (gene -> column map of g
 *                           int32) over their columns, a barrier, one coalesced store.  Z has the dense layout, so
 *                           mi_prep_fetch_scaled, k_prep_gram and k_prep_project run unchanged.
 *
 * Cell QC (mi_prep_cell_qc), on the counts of either kind of handle:
 *   k_prep_cell_qc          one wavefront per cell, k_prep_normalize's walk: the lane-strided fp64 total and the same butterfly
 *                           (n_count is bit for bit the total the normaliser divides by), the same walk over the masked
 *                           genes (subset_count), an integer wave reduction over x != 0 (n_feature).
 *   k_prep_csr_cell_qc      k_prep_csr_normalize's order: each entry to lane `column & 63`, columns ascending; a stored
 *                           zero is no feature.
 *
 * Regression (mi_prep_select_regressed): Z = the scaled residuals of y ~ design, for vars.to.regress.  Stage 1 gathers the
 * chosen columns of Y into Z unscaled, with the two select kernels (mu = 0, inv = 1, an infinite clip:
 * fminf((y - 0) * 1, inf) is y); every later stage reads the dense Z alone, so a sparse handle gives the bits of a dense
 * one.  Q: n x q row-major fp64, an orthonormal basis of the design.  The kernels have k_prep_col_partial's shape and
 * order (the moments are that kernel itself): a workgroup is 64 columns x 4 row lanes over a slice of MI_PREP_ROW_SLICE rows; lane ty (one wavefront, so its row
 * of Q is uniform) adds rows r0 + ty, r0 + ty + 4, ... ascending; the four lanes meet in LDS as ((s0 + s1) + s2) + s3;
 * k_prep_col_finish adds the slices in ascending order.  Every product is a separate multiply and add (no contraction).
 *   k_prep_regress_coef     c_kj = sum_i Q_ik (double) y_ij and S_j = sum_i (double) y_ij^2.
 *   k_prep_col_partial<RegressMoment>  mean_j = (sum_i r_ij) / n, then ss_j = sum_i (r_ij - mean_j)^2, var_j = ss_j / (n - 1); r is
 *                           recomputed each time as (double) y - acc with acc = Q_i0 c_0, then acc = acc + Q_ik c_k for k
 *                           ascending: no n x h fp64 buffer exists.
 *   host, inside the entry  flat_j = ss_j <= 1e-16 S_j (a convention of this package: an all-zero gene, a constant gene and
 *                           a gene in the span of the design leave a residual that is fp64 noise of order n 2^-53 relative
 *                           to y, which 1 / sd would scale up to the clip; 1e-8 rms(y) is three decades above that noise at
 *                           n = 10^5 and far below any real residual); inv_j = 1.0 / sqrt(var_j) in fp64.
 *   k_prep_regress_scale    in place: z = flat ? 0 : (float) fmin((r - mean) * inv, clip), fp64 with one rounding to f32.
 *
 * SCTransform (mi_prep_gene_log1p_sum, mi_prep_nb_fit, mi_prep_sct_residual_moments, mi_prep_sct_select; DESIGN.md section 5c
 * "SCTransform").  The chain is this package's specification, modelled on sctransform::vst; it is unpinned against R.
 *   k_prep_col_partial<ColLog1p>  sum_i log1p((double) x_ij): the SUM mode's walk with another term, dense and sparse (a zero adds
 *                           +0.0 either way), for sctransform's geometric mean.
 *   k_sct_gather            the counts of the fit cells x fit genes as a dense f32 block, gene-major (one thread per element);
 *   k_sct_csr_gather        the same from CSR: one workgroup per fit cell, its row in LDS (zeros, a barrier, the stored entries
 *                           of fit genes over them).  The fit reads the block alone: a sparse handle gives a dense one's bits.
 *   k_sct_nb_fit            one workgroup of 256 threads per gene.  The gene's counts sit in LDS (MI_PREP_SCT_MAX_FIT_CELLS
 *                           floats, 32 KB, + 160 B for the sums), the centred covariate xc is one fp64 array shared by all genes;
 *                           mu = exp(b0 + b1 xc) is recomputed in every pass, nothing per cell is kept between rounds.  Every sum
 *                           is per thread over the cells t, t + 256, ... ascending, then the wave butterfly, then the four waves
 *                           in LDS as ((s0 + s1) + s2) + s3: no atomics, two runs are bit-identical.  Every thread computes the
 *                           scalar logic of a round from the same sums, so control flow is workgroup-uniform.  psi and psi' are
 *                           csrc/mi_sct_math.h.  The model is y ~ NB(mu, alpha), variance mu + alpha mu^2, theta = 1 / alpha:
 *                             1. Poisson start: mu = y + 0.1, eta = log mu, then 8 IRLS steps with w = mu, z = eta + (y - mu) / mu,
 *                                each the closed form of the 2 x 2 weighted normal equations (5 sums).
 *                             2. Poisson rule, once: T = sum (y - mu)^2 - y; T <= 0: alpha = 0, poisson = 1, only b moves below;
 *                                else alpha = T / sum mu^2.
 *                             3. at most 40 rounds.  s = sum (psi(y + theta) - psi(theta)) + log1p(-mu / (theta + mu)) - (y - mu) /
 *                                (theta + mu) and s' = sum (psi'(y + theta) - psi'(theta)) + mu / (theta (theta + mu)) + (y - mu) /
 *                                (theta + mu)^2 (the derivatives of the log-likelihood in theta, each bracket a small difference
 *                                taken first); l1 = -theta^2 s, l2 = theta^4 s' + 2 theta^3 s.  l2 < 0: alpha' = alpha - l1 / l2,
 *                                else 2 alpha if l1 > 0 and alpha / 2 if not; a proposal that is not > 0 becomes alpha / 4; then
 *                                alpha' is limited to [alpha / 8, 8 alpha].  One Fisher-scoring step of b at alpha' and the old
 *                                mu: U = sum (y - mu) / (1 + alpha' mu) [1, xc], I = sum w [1, xc]^T [1, xc], w = mu / (1 + alpha'
 *                                mu), b += I^-1 U.  lambda^2 = U^T I^-1 U + l1^2 / (-l2) (infinite while l2 >= 0): the squared
 *                                distance to the optimum in standard errors.  A gene with lambda^2 <= 1e-16 takes the update and
 *                                stops, converged = 1; after 40 rounds it keeps its last iterate, converged = 0.
 *                             4. se_b0c = sqrt(I_11 / det I), se_b1 = sqrt(I_00 / det I), se_alpha = 1 / sqrt(-l2) of the last
 *                                round (NaN for a Poisson gene or while l2 >= 0).
 *   k_prep_col_partial<SctMoment>  the column reduction on r = clip((x - mu) / sqrt(mu + alpha mu^2), +-clip), mu = exp(b0 +
 *                           b1 log_umi_i): the sum, then the squares about the mean;
 *   k_prep_csc_row_partial<SctMoment>  the same on the transpose.  A zero's residual depends on the cell, so every row of
 *                           the slice is computed, and the contract holds bit for bit.
 *   k_sct_select            Z = (float) r for the chosen genes, k_prep_select's shape;
 *   k_prep_csr_select<SctCols>  the zeros' residuals fill the cell's LDS row, the stored entries overwrite.
 */
#ifndef MI_PREP_H
#define MI_PREP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_prep_matrix mi_prep_matrix;

#define MI_PREP_MAX_CELLS    (1 << 23)      /* n: the row slices of the column reductions are one grid dimension */
#define MI_PREP_MAX_ENTRIES  (1ll << 32)    /* n * g (16 GiB of f32 per matrix; counts and normalised are both resident) */
#define MI_PREP_MAX_NNZ      2147483647ll   /* stored entries of a sparse handle: positions stay 32-bit */
#define MI_PREP_MAX_FEATURES 4096           /* h of mi_prep_select (G: 128 MiB of fp64) */
#define MI_PREP_MAX_PCS      128            /* p of mi_prep_project */
#define MI_PREP_ROW_SLICE    256            /* rows per partial sum of the column reductions */
#define MI_PREP_GRAM_CHUNK   512            /* cells whose products accumulate in f32 before the fp64 sum over chunks */
#define MI_PREP_GRAM_WORKSPACE (256ll << 20)  /* bytes of f32 chunk tiles in flight in mi_prep_gram: more chunks take more passes */
#define MI_PREP_MAX_DESIGN_COLS 9           /* q of mi_prep_select_regressed: the intercept + 8 covariates */
#define MI_PREP_SCT_MAX_FIT_CELLS 8192      /* cells of mi_prep_nb_fit: a gene's counts are 32 KB of LDS */

/* X: n x g row-major counts (any non-negative finite values).  Uploads X to `device`.  MI_EINVAL for NULL arguments,
 * n < 2, g < 1, a NaN, an infinity or a negative value; MI_EUNSUPPORTED for n > MI_PREP_MAX_CELLS or
 * n * g > MI_PREP_MAX_ENTRIES. */
int mi_prep_create_f32(const float *X, int n, int g, int device, mi_prep_matrix **out);
/* The same matrix as CSR: indptr n + 1 entries, indices and data indptr[n] entries.  Checks everything, transposes on the
 * host (one counting sort), uploads.  MI_EINVAL for NULL arguments, n < 2, g < 1, indptr[0] != 0, a decreasing indptr, a
 * column outside [0, g), columns of a row not strictly ascending, a NaN, infinite or negative value; MI_EUNSUPPORTED for
 * n > MI_PREP_MAX_CELLS or indptr[n] > MI_PREP_MAX_NNZ.  n * g is not limited.  A stored zero is legal and behaves as an
 * absent entry in every result (it keeps its place in mi_prep_fetch_normalized_csr, with the value 0). */
int mi_prep_create_csr_f32(const int64_t *indptr, const int32_t *indices, const float *data, int n, int g, int device,
                           mi_prep_matrix **out);
int mi_prep_destroy(mi_prep_matrix *m);
/* Either kind of handle; every output is nullable.  nnz: the stored entries of a sparse handle, n * g for a dense one.
 * device_bytes: what the handle holds resident on the device now (the scratch of a running pass is not the handle's). */
int mi_prep_info(const mi_prep_matrix *m, int *n, int *g, int64_t *nnz, int *sparse, int64_t *device_bytes);

/* Seurat's LogNormalize: per-cell totals in fp64, y = (float) log1p((double) x * scale_factor / total), kept as a second
 * device-resident matrix (a second call replaces it).  A cell whose total is 0 keeps all zeros (Seurat divides by the
 * zero total and returns NaN for that cell).  MI_EINVAL unless scale_factor is finite and > 0. */
int mi_prep_normalize(mi_prep_matrix *m, double scale_factor, float *out_kernel_ms);
/* out: n x g.  MI_ESTATE before mi_prep_normalize; MI_EUNSUPPORTED on a sparse handle. */
int mi_prep_fetch_normalized(mi_prep_matrix *m, float *out);
/* out_data: the normalised values of the stored entries, in the caller's CSR order (indptr[n] entries).  MI_EINVAL on a
 * dense handle, MI_ESTATE before mi_prep_normalize.  Every other pass below serves both kinds of handle. */
int mi_prep_fetch_normalized_csr(mi_prep_matrix *m, float *out_data);

/* which: 0 = counts, 1 = normalised matrix (MI_ESTATE before mi_prep_normalize).  Per gene, in fp64, two passes: mean =
 * (sum of x) / n, then var = (sum of (x - mean)^2) / (n - 1); nnz = cells with x != 0.  Outputs: g entries each, nullable. */
int mi_prep_gene_stats(mi_prep_matrix *m, int which, double *mean, double *var, int32_t *nnz, float *out_kernel_ms);

/* The second pass of Seurat's `vst`, on the counts: out[j] = sum_i min((x_ij - mean_j) / sd_j, clip)^2 / (n - 1) in fp64,
 * 0 where sd_j == 0.  mean, sd, out: g entries.  MI_EINVAL for a non-finite mean, a negative or non-finite sd, a NaN clip. */
int mi_prep_clipped_variance(mi_prep_matrix *m, const double *mean, const double *sd, double clip, double *out,
                             float *out_kernel_ms);

/* Gathers the h chosen columns of the normalised matrix (any order; MI_EINVAL for an index outside [0, g) or a repeated
 * one, h < 1, a non-finite mu, a negative or non-finite sigma, clip NaN or <= 0) and materialises the scaled matrix once:
 *     z = fminf((y - (float) mu) * (float) (1.0 / sigma), (float) clip),     z = 0 where sigma == 0
 * (separate f32 subtract and multiply, no contraction).  mu, sigma: h entries, in the order of `genes`.  MI_EUNSUPPORTED
 * for h > MI_PREP_MAX_FEATURES; MI_ESTATE before mi_prep_normalize.  mi_prep_fetch_scaled (out: n x h), mi_prep_gram and
 * mi_prep_project all read this one Z: what the products consume is bit for bit what the caller can fetch. */
int mi_prep_select(mi_prep_matrix *m, const int32_t *genes, int h, const double *mu, const double *sigma, double clip,
                   float *out_kernel_ms);
int mi_prep_fetch_scaled(mi_prep_matrix *m, float *out);

/* Per cell, on the counts (no mi_prep_normalize needed): n_count = the fp64 total (the one mi_prep_normalize divides by),
 * n_feature = genes with x != 0, subset_count = the total over the genes with gene_mask[j] == 1 (Seurat's nCount_RNA,
 * nFeature_RNA and the numerator of PercentageFeatureSet).  gene_mask: g bytes, nullable; outputs: n entries each,
 * nullable.  MI_EINVAL for a NULL handle, a mask byte other than 0 or 1, subset_count without a mask. */
int mi_prep_cell_qc(mi_prep_matrix *m, const uint8_t *gene_mask, double *n_count, int32_t *n_feature, double *subset_count,
                    float *out_kernel_ms);

/* mi_prep_select on the residuals of a linear model (ScaleData(vars.to.regress)): with y the chosen column of the
 * normalised matrix, r = y - Q (Q^T y), z = (float) fmin((r - mean(r)) / sd(r), clip) (sd with n - 1), z = 0 for a flat
 * column (see above).  Q: n x q row-major, an orthonormal basis of [1, covariates]; orthonormality is the caller's
 * contract, the entry computes the expression whatever Q is.  Z has mi_prep_select's layout, so mi_prep_fetch_scaled,
 * mi_prep_gram and mi_prep_project follow unchanged.  Outputs, each nullable: out_coef q x h (Q^T y), out_mean, out_var
 * (of the residuals) and out_flat, h entries each, in the order of `genes`.  All checks before any device work: MI_EINVAL
 * for a NULL argument, h < 1, q < 1, a gene outside [0, g) or chosen twice, a non-finite Q entry, clip NaN or <= 0;
 * MI_EUNSUPPORTED for h > MI_PREP_MAX_FEATURES or q > MI_PREP_MAX_DESIGN_COLS; MI_ESTATE before mi_prep_normalize.  A
 * failure leaves nothing selected (mi_prep_fetch_scaled: MI_ESTATE). */
int mi_prep_select_regressed(mi_prep_matrix *m, const int32_t *genes, int h, const double *Q, int q, double clip,
                             double *out_coef, double *out_mean, double *out_var, uint8_t *out_flat, float *out_kernel_ms);

/* out[j] = sum_i log1p((double) x_ij) over the counts, fp64, g entries: sctransform's geometric mean of a gene is
 * expm1(out[j] / n).  The order of mi_prep_gene_stats' sum. */
int mi_prep_gene_log1p_sum(mi_prep_matrix *m, double *out, float *out_kernel_ms);

/* The negative-binomial regression of SCTransform's step 1 (k_sct_nb_fit above): for each of the g1 `genes`, over the mc
 * `cells` (any order, no repeats), y ~ NB(mu, alpha) with log mu = b0 + b1 log_umi.  log_umi: mc entries, in the order of
 * `cells` (log10 of the cell's total count); the kernel regresses on log_umi - mean, the mean being the sum in that order
 * divided by mc.  Outputs, g1 entries each, all required: b0 (on the uncentred covariate: b0c - b1 mean), b1, alpha, the
 * standard errors se_b0c (of the centred intercept), se_b1, se_alpha (NaN for a Poisson gene), iterations (rounds of step
 * 3), converged, poisson.  Natural-log coefficients.  MI_EINVAL for a NULL argument, a cell outside [0, n) or a gene outside
 * [0, g) or either repeated, mc < 3, g1 < 1, a non-finite log_umi (a cell without counts), a log_umi that is the same in
 * every cell; MI_EUNSUPPORTED for mc > MI_PREP_SCT_MAX_FIT_CELLS or g1 > MI_PREP_MAX_FEATURES.  Needs no mi_prep_normalize. */
int mi_prep_nb_fit(mi_prep_matrix *m, const int32_t *cells, int mc, const int32_t *genes, int g1, const double *log_umi,
                   double *out_b0, double *out_b1, double *out_alpha, double *out_se_b0c, double *out_se_b1,
                   double *out_se_alpha, int32_t *out_iterations, uint8_t *out_converged, uint8_t *out_poisson,
                   float *out_kernel_ms);

/* Per chosen gene, over all n cells: mean and variance (n - 1, about that mean, two passes, fp64) of the Pearson residual
 *     r = min(max((x - mu) / sqrt(mu + alpha mu^2), -clip), clip),     mu = exp(b0 + b1 log_umi_i).
 * b0, b1, alpha, out_mean, out_var: gp entries in the order of `genes`; log_umi: n entries.  MI_EINVAL for a NULL argument,
 * gp < 1 or > g, a gene outside [0, g) or repeated, a non-finite b0, b1 or log_umi, alpha negative or not finite, clip NaN
 * or <= 0. */
int mi_prep_sct_residual_moments(mi_prep_matrix *m, const int32_t *genes, int gp, const double *b0, const double *b1,
                                 const double *alpha, const double *log_umi, double clip, double *out_mean, double *out_var,
                                 float *out_kernel_ms);

/* SCTransform's scale.data: Z = (float) r (above, clipped at +-clip) for the h chosen genes, then stages 2 - 5 of
 * mi_prep_select_regressed on that Z with unit scale and no further clip: z = flat ? 0 : (float) (r - Q (Q^T r) - mean).
 * With Q the basis of [1] this is centring (do.center = TRUE, do.scale = FALSE); with [1, covariates] vars.to.regress.
 * Arguments, outputs and the flat rule as mi_prep_select_regressed; the same checks, and those of
 * mi_prep_sct_residual_moments on the parameters; MI_EUNSUPPORTED for h > MI_PREP_MAX_FEATURES or q >
 * MI_PREP_MAX_DESIGN_COLS.  Q = NULL with q = 0 stops after stage 1: Z holds the clipped residuals themselves, uncentred, and
 * the four outputs are not written.  Needs no mi_prep_normalize.  A failure leaves nothing selected. */
int mi_prep_sct_select(mi_prep_matrix *m, const int32_t *genes, int h, const double *b0, const double *b1, const double *alpha,
                       const double *log_umi, double clip, const double *Q, int q, double *out_coef, double *out_mean,
                       double *out_var, uint8_t *out_flat, float *out_kernel_ms);

/* SCTransform's corrected counts and its `data` slot as a second handle (modelled on sctransform::correct_counts; unpinned
 * against R).  For a listed gene with (b0, b1, alpha), a cell with lu = log_umi[i] and the stored count x, all in fp64:
 *     mu   = exp(b0 + b1 lu)              s   = sqrt(mu + alpha (mu mu))
 *     mu_r = exp(b0 + b1 log_umi_ref)     s_r = sqrt(mu_r + alpha (mu_r mu_r))
 *     r = ((double) x - mu) / s (not clipped)       c = fmax(rint(mu_r + r s_r), 0.0)   (a multiply, an add, half to even)
 *     corrected = (float) c               data = (float) log1p(c)
 * (mi_sct::corrected_count, csrc/mi_sct_math.h: the one text every kernel form calls).  A gene that is not listed gives all
 * zeros: the output keeps the g columns of `m`, so gene names stay aligned (a convention of this package).  The caller
 * passes log10 of the median of the cells' totals as log_umi_ref.
 * *out: a new, independent handle on m's device, of m's kind and shape: its counts are the corrected counts, its normalised
 * matrix is the data slot (every `which = 1` pass works at once; mi_prep_normalize would replace it).  m is not modified
 * (its device_bytes is the same before and after), may be destroyed first, and all scratch is freed on return.
 *   dense handle   k_sct_correct writes both matrices element by element; mu_r and s_r are computed once per gene
 *                  (k_sct_gene_table).
 *   sparse handle  a corrected zero need not stay zero, so the output has its own structure, built on the device with no
 *                  n x g buffer.  It holds exactly the entries with c != 0 (a stored zero or an absent entry of m is x = 0; a
 *                  stored entry whose c is 0 is dropped).  k_sct_csr_rows, one workgroup per cell: by chunk of 4096 genes the
 *                  zeros' values fill the cell's LDS row (32 KB of fp64) and the stored entries overwrite; a count launch,
 *                  k_prep_scan_counts into indptr, then a fill launch that evaluates again and writes columns (ascending),
 *                  counts and data by an ordered compaction (ballot and lane prefix inside a wavefront, the four wavefronts'
 *                  counts through LDS).  The transpose is a two-level counting sort of that CSR, which evaluates nothing:
 *                  k_csr_block_hist counts the entries per (block of R rows, gene) (integer atomics: any order gives the same
 *                  counts; blocks x genes int32 of scratch, at most 2^26), k_csr_block_offsets makes each gene's counts the
 *                  prefix over the blocks, k_prep_scan_counts gives colptr, and k_csr_block_transpose, one workgroup per
 *                  block, walks its rows one after another (a row's columns are distinct; a barrier parts the rows), so a
 *                  gene's cells ascend and the position map is the entry's place in the CSR.  The other form -- a second
 *                  evaluation gene-major over m's transpose -- measured twice as slow (profiles/prep_sct_correct_transpose_ab.json).
 *                  Integer counts and ordered stores only: two runs are bit-identical and the result is that of the dense
 *                  handle on the densified input.
 * All checks before any device work, those of mi_prep_sct_residual_moments on the parameters: MI_EINVAL for a NULL argument,
 * gp < 1 or > g, a gene outside [0, g) or repeated, a non-finite b0, b1, log_umi or log_umi_ref, alpha negative or not
 * finite.  Found on the device, with no handle created: MI_EINVAL for a c that is not finite (an overflowed or vanished mu;
 * a flag the kernels raise), MI_EUNSUPPORTED for more than MI_PREP_MAX_NNZ output entries on a sparse handle (the scanned
 * total).  Needs no mi_prep_normalize. */
int mi_prep_sct_correct(mi_prep_matrix *m, const int32_t *genes, int gp, const double *b0, const double *b1,
                        const double *alpha, const double *log_umi, double log_umi_ref, mi_prep_matrix **out,
                        float *out_kernel_ms);
/* out: the counts of a dense handle, n x g.  MI_EUNSUPPORTED on a sparse handle. */
int mi_prep_fetch_counts(mi_prep_matrix *m, float *out);
/* The structure of a sparse handle and its counts: indptr n + 1 entries, indices and data `nnz` of mi_prep_info; each output
 * is nullable.  MI_EINVAL on a dense handle. */
int mi_prep_fetch_csr(mi_prep_matrix *m, int64_t *indptr, int32_t *indices, float *data);

/* out_G: h x h fp64, G = Z^T Z (not divided by n - 1).  Every entry is the fp64 sum, in chunk order, of the f32 fmaf chains
 * over the cells of each chunk of MI_PREP_GRAM_CHUNK cells.  MI_ESTATE before mi_prep_select. */
int mi_prep_gram(mi_prep_matrix *m, double *out_G, float *out_kernel_ms);

/* out = Z V: V is h x p row-major f32 (finite), out n x p; every entry one f32 fmaf chain over the h features in order.
 * MI_EINVAL for p < 1, MI_EUNSUPPORTED for p > MI_PREP_MAX_PCS, MI_ESTATE before mi_prep_select. */
int mi_prep_project(mi_prep_matrix *m, const float *V, int p, float *out, float *out_kernel_ms);

#define MI_PREP_MARKERS_COUNTS     0   /* the uploaded values */
#define MI_PREP_MARKERS_NORMALIZED 1   /* the output of mi_prep_normalize */
#define MI_PREP_MARKERS_GATHER_INPLACE 4u   /* flags bit 2: a sparse handle reads its values through the position map */
#define MI_PREP_MARKERS_GATHER_PERMUTE 8u   /* flags bit 3: ... from a gene-major copy made first (nnz floats of scratch) */

/* The rank-sum marker pass of mi_metrics.h (mi_rank_sum_markers_f32: the same L, B, K, outputs, label rules, limits and the
 * flags MI_MARKERS_SUM_PLAIN and MI_MARKERS_GLOBAL) on the matrix the handle holds on the device, with no upload: `which`
 * picks the uploaded values or the normalised ones; n and g are the handle's.  Every output equals, bit for bit, that of
 * mi_rank_sum_markers_f32 on the same (densified) matrix.  The handle is not modified and all scratch is freed on return:
 * mi_prep_info's device_bytes is the same before and after.
 *   dense handle   the kernels of mi_rank_sum_markers_f32 on the resident matrix; the per-gene non-zero counts its host scan
 *                  gives come from k_markers_count (csrc/markers_kernels.hip).
 *   sparse handle  no transpose and no n x g buffer: gene j's candidates are its stored entries (cells rows[k] ascending,
 *                  values V[pos[k]]).  A stored zero is a zero: the compaction skips it, it joins the zero block, and
 *                  zeros = n - (true non-zeros).  The launch (LDS capacity, slab stride, LDS or HBM form per gene) is
 *                  planned from the stored counts, an upper bound read from colptr; the true non-zero count comes out of the
 *                  compaction and the sort is padded to its power of two.  The sums walk the stored entries in
 *                  ascending cell order, one thread per (gene, labelling): the dense kernel's additions in its order.
 *                  The two GATHER flags pick how the values are read (neither: the form kept by measurement, DESIGN.md
 *                  section 5c; they change no result and a dense handle ignores them).
 * All checks before any device work, in this order: MI_EINVAL for NULL m, L or out_rank2, `which` outside {0, 1}, B < 1, K
 * outside [1, 64], unknown flags or both GATHER flags, a label >= K; MI_ESTATE for which == 1 before mi_prep_normalize;
 * MI_EUNSUPPORTED for n > MI_MARKERS_MAX_CELLS and for B * g * K > MI_MARKERS_MAX_ENTRIES. */
int mi_prep_rank_sum_markers(mi_prep_matrix *m, int which, const uint16_t *L, int B, int K, uint32_t flags,
                             int64_t *out_rank2, int32_t *out_npos, double *out_sum, int64_t *out_tie,
                             float *out_kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* MI_PREP_H */
